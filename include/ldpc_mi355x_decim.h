/* ldpc_mi355x_decim.h -- the entry points of the guided-decimation min-sum decoder.  A part of ldpc_mi355x.h, which
 * includes it at the end of its ldpc_decim_* section (THE RULE, the options struct and every status are stated there):
 * include that header, not this one.  Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by
 * symbol lookup. */
#ifndef LDPC_MI355X_DECIM_H
#define LDPC_MI355X_DECIM_H

#ifndef LDPC_MI355X_H
#error "include ldpc_mi355x.h, which includes this file"
#endif

ldpc_status ldpc_decim_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                              const float *channel_llr, int64_t round_iters, int64_t max_decimations,
                              const ldpc_decim_options *options, ldpc_decim_decoder **out);
ldpc_status ldpc_decim_destroy(ldpc_decim_decoder *dec);
int32_t ldpc_decim_kernel(const ldpc_decim_decoder *dec);
int32_t ldpc_decim_tile_syndromes(const ldpc_decim_decoder *dec);
int32_t ldpc_decim_last_grid(const ldpc_decim_decoder *dec);
ldpc_status ldpc_decim_decode_batch(ldpc_decim_decoder *dec, int64_t batch, const uint8_t *syndromes, uint8_t *errors,
                                    uint8_t *converged, double *llr, int32_t *iters, int32_t *decimated);
ldpc_status ldpc_decim_decode_batch_device(ldpc_decim_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                           uint8_t *d_errors, uint8_t *d_converged, double *d_llr, int32_t *d_iters,
                                           int32_t *d_decimated, void *stream);

#endif /* LDPC_MI355X_DECIM_H */
