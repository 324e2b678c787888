/* ldpc_mi355x_osd_search.h -- the entry points that put an `ldpc_osd` handle on the STANDARD RULE of the
 * ordered-statistics step.  A part of ldpc_mi355x.h, which includes it at the end of its BP+OSD section (the rule and
 * every status are stated there): include that header, not this one.  Added WITHOUT a change of
 * LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup. */
#ifndef LDPC_MI355X_OSD_SEARCH_H
#define LDPC_MI355X_OSD_SEARCH_H

#ifndef LDPC_MI355X_H
#error "include ldpc_mi355x.h, which includes this file"
#endif

ldpc_status ldpc_osd_set_search(ldpc_osd *osd, int32_t method, int64_t order, int64_t n, const double *channel_llr);
int32_t ldpc_osd_search_method(const ldpc_osd *osd);
int64_t ldpc_osd_search_weight(const ldpc_osd *osd, int64_t j);

#endif /* LDPC_MI355X_OSD_SEARCH_H */
