/* ldpc_mi355x_stab_debug.h -- the test hook of the stabilizer min-sum decoder.  A part of ldpc_mi355x_debug.h, which
 * includes it where the hook is described: include that header, not this one.  Not part of the boundary. */
#ifndef LDPC_MI355X_STAB_DEBUG_H
#define LDPC_MI355X_STAB_DEBUG_H

#ifndef LDPC_MI355X_DEBUG_H
#error "include ldpc_mi355x_debug.h, which includes this file"
#endif

ldpc_status ldpc_debug_stab_tile_plan(int64_t r, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                      int32_t *tile_syndromes, int64_t *state_bytes);

#endif /* LDPC_MI355X_STAB_DEBUG_H */
