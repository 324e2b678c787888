/* ldpc_mi355x_pauli_relay.h -- the entry points of the Pauli relay min-sum decoder.  A part of ldpc_mi355x.h, which
 * includes it at the end of its ldpc_pauli_relay_* section (THE RULE, the options struct and every status are stated there):
 * include that header, not this one.  Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by
 * symbol lookup. */
#ifndef LDPC_MI355X_PAULI_RELAY_H
#define LDPC_MI355X_PAULI_RELAY_H

#ifndef LDPC_MI355X_H
#error "include ldpc_mi355x.h, which includes this file"
#endif

ldpc_status ldpc_pauli_relay_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz, const float *prior_x,
                                    const float *prior_y, const float *prior_z, int64_t legs, const float *gammas,
                                    const int32_t *leg_iters, const ldpc_pauli_relay_options *options,
                                    ldpc_pauli_relay_decoder **out);
ldpc_status ldpc_pauli_relay_destroy(ldpc_pauli_relay_decoder *dec);
int32_t ldpc_pauli_relay_kernel(const ldpc_pauli_relay_decoder *dec);
int32_t ldpc_pauli_relay_tile_syndromes(const ldpc_pauli_relay_decoder *dec);
int32_t ldpc_pauli_relay_last_grid(const ldpc_pauli_relay_decoder *dec);
ldpc_status ldpc_pauli_relay_decode_batch(ldpc_pauli_relay_decoder *dec, int64_t batch, const uint8_t *sx, const uint8_t *sz,
                                          uint8_t *gx, uint8_t *gz, uint8_t *converged, double *llr, int32_t *iters,
                                          int32_t *solutions);
ldpc_status ldpc_pauli_relay_decode_batch_device(ldpc_pauli_relay_decoder *dec, int64_t batch, const uint8_t *d_sx,
                                                 const uint8_t *d_sz, uint8_t *d_gx, uint8_t *d_gz, uint8_t *d_converged,
                                                 double *d_llr, int32_t *d_iters, int32_t *d_solutions, void *stream);

#endif /* LDPC_MI355X_PAULI_RELAY_H */
