/* ldpc_mi355x_stab.h -- the joint Pauli min-sum decoder of a general (non-CSS) stabilizer code: THE RULE, the options
 * struct and the entry points.  A part of ldpc_mi355x.h, which includes it after its ldpc_pauli_relay_* section: include
 * that header, not this one.  Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol
 * lookup.
 *
 * ldpc_pauli_minsum_* decodes a CSS code: every check is all-X or all-Z.  Here a check may mix Pauli types (the five-qubit
 * code, the XZZX surface code, a Clifford-deformed CSS code: what a stabilizer tableau holds).  Every qubit carries the
 * three beliefs of the Pauli decoder; every EDGE of the graph has a type, the Pauli the stabilizer has on that qubit, and
 * the scalar min-sum message of an edge speaks about "the error on this qubit anticommutes with that Pauli".  Compare, add
 * and one multiply in binary32, no division and no transcendental function: THE RULE has one legal outcome in IEEE
 * binary32 and a numpy model equals the device in every bit, LLRs included.  Flooding schedule only.  Not a decoder of
 * the reference.
 *
 * Inputs.  sx_part and sz_part: two zero-based CSC patterns over the same n qubits (ldpc_css_pattern), each with the same
 * r >= 1 rows.  sx_part stores (i, j) where stabilizer i has X or Y on qubit j, sz_part where it has Z or Y.  Edge (i, j)
 * exists if either pattern stores it; its type is X (only sx_part), Z (only sz_part) or Y (both).  prior_x[n], prior_y[n],
 * prior_z[n], alpha, clip, max_iters: as ldpc_pauli_minsum_create takes them.  Syndromes s [batch][r]: s_i is the XOR over
 * the edges of check i of ez_j (X-type edge), ex_j (Z-type) or ex_j ^ ez_j (Y-type) -- whether the error anticommutes with
 * the stabilizer; an entry that is not 0 counts as 1.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * min(x, y) below means  x < y ? x : y  with the operands in the order given.
 * State per syndrome: three totals MX[j], MY[j], MZ[j] -- the sum of the messages of the qubit's X-, Y- and Z-type edges --
 * initially +0; the check-to-qubit messages c[i][j], initially +0.
 * Derived, wherever used (a belief for W contains the totals of the edge types W anticommutes with):
 *     GX[j] = (prior_x[j] + MZ[j]) + MY[j];   GY[j] = (prior_y[j] + MZ[j]) + MX[j];   GZ[j] = (prior_z[j] + MX[j]) + MY[j].
 * For t = 1 .. max_iters:
 *   1. Check sweep.  For check i with its qubits j_0 < j_1 < ... (ascending), with G of j_k, by the type of edge (i, j_k):
 *        X-type:  u_k = min(GY, GZ);  w_k = GX < 0 ? GX : +0
 *        Z-type:  u_k = min(GY, GX);  w_k = GZ < 0 ? GZ : +0
 *        Y-type:  u_k = min(GX, GZ);  w_k = GY < 0 ? GY : +0
 *        b_k = min(max((u_k - c[i][j_k]) - w_k, -clip), clip);   neg_k = (b_k < 0);   mag_k = |b_k|
 *        m1, m2, a, par and the new c[i][j_k] exactly as in step 1 of THE RULE of ldpc_minsum_*: par starts from the check's
 *        syndrome entry s_i; the new message is alpha * (k == a ? m2 : m1) with its sign bit set iff par XOR neg_k.  All
 *        b_k are formed from the old state before any message is replaced.  A check with no qubits sends nothing.
 *   2. Bit sweep.  MX[j] = ((+0 + c[i_0][j]) + c[i_1][j]) + ... over the X-type edges of j in ascending check order; MY[j]
 *      and MZ[j] the same sums over its Y-type and its Z-type edges.  Decision, as ldpc_pauli_minsum_*:  best = X, g = GX;
 *      if GZ < g { best = Z, g = GZ };  if GY < g { best = Y, g = GY };  E = (g <= 0) ? best : I;  ex[j] = (E is X or Y);
 *      ez[j] = (E is Z or Y).
 *   3. Stop test.  If for every check the XOR over its edges of ez_j (X-type), ex_j (Z-type), ex_j ^ ez_j (Y-type) equals
 *      its syndrome entry (an empty check is matched only by a 0 entry): converged = 1, iters = t, stop; the totals, ex and
 *      ez stay as they are.
 * Not stopped after max_iters: converged = 0, iters = max_iters.  With finite inputs no NaN or infinity can arise.
 *
 * Outputs.  gx [batch][n] uint8 = ex, gz [batch][n] uint8 = ez; converged [batch] uint8; iters [batch] int32 (may be
 * NULL); llr [batch][3][n] DOUBLE (may be NULL): the planes GX, GY, GZ of the final state widened exactly -- the layout of
 * ldpc_pauli_minsum_*, so ldpc_css_trials_score* reads the guesses.  max_iters = 0: zeros everywhere, llr included.
 * batch = 0: LDPC_OK, nothing touched.
 *
 * Consequence.  On a CSS input -- the Hx rows as X-type edges, then the Hz rows as Z-type edges, s = [sx | sz] -- every
 * output equals ldpc_pauli_minsum_* in every bit: MX is that rule's TZ, MZ its TX, and with no Y-type edge MY stays +0.
 * The sum (prior_x + MZ) is never -0, because a total starts from +0 (x + y is -0 only for two -0 operands), so adding
 * MY = +0 to it changes no bit; the same holds for GZ, and GY is that rule's (prior_y + TX) + TZ as it stands.
 *
 * ldpc_stab_minsum_kernel: 1 = on-chip (MX, MY, MZ, the check records and the syndromes of the S <= 64 syndromes a workgroup
 * holds live in LDS for the whole decode; needs (4 (3 n + record words) + r) bytes <= 159 KiB for one syndrome, records as
 * in ldpc_minsum_kernel); 2 = unlimited (tiles of 64 syndromes in a workspace the handle owns); 0 for NULL.
 * options->kernel_variant 0 = by size, 1 / 2 force a tier (1 where the state does not fit: LDPC_ERR_UNSUPPORTED).
 * ldpc_stab_minsum_tile_syndromes and ldpc_stab_minsum_last_grid: as ldpc_minsum_tile_syndromes and ldpc_minsum_last_grid, by
 * the same policy over that state.
 *
 * ldpc_stab_minsum_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for everything
 * ldpc_pauli_minsum_create refuses (a NULL or non-finite prior, alpha outside (0, 1], clip not in (0, inf), a kernel_variant
 * outside 0..2, a NULL pattern or one ldpc_bp_create rejects; the message names the argument), for patterns whose row counts
 * differ and for r < 1; a union of 2^28 or more edges, checks or qubits: LDPC_ERR_UNSUPPORTED; without a device
 * LDPC_ERR_NO_DEVICE.  The library does not check that the stabilizers commute.  The decode entries reject a NULL handle, a
 * negative batch and a NULL required pointer the same way.  ldpc_stab_minsum_decode_batch takes HOST buffers and is
 * synchronous (its wait is bounded by ldpc_set_wait_limit_ms); ldpc_stab_minsum_decode_batch_device takes DEVICE pointers
 * and is asynchronous on `stream`; calls on one handle run in call order whatever streams they are given. */
#ifndef LDPC_MI355X_STAB_H
#define LDPC_MI355X_STAB_H

#ifndef LDPC_MI355X_H
#error "include ldpc_mi355x.h, which includes this file"
#endif

typedef struct ldpc_stab_minsum_decoder ldpc_stab_minsum_decoder;

/* Optional; pass NULL to ldpc_stab_minsum_create for defaults.  A zeroed struct means defaults too, except `device` (0 is
 * device 0; -1 = the current one): alpha = 0 / clip = 0 select 0.75 / 1.0e6f. */
typedef struct ldpc_stab_minsum_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the qubit-to-check values, finite, > 0; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_stab_minsum_kernel */
    int32_t reserved[12];
} ldpc_stab_minsum_options;

ldpc_status ldpc_stab_minsum_create(int64_t n, const ldpc_css_pattern *sx_part, const ldpc_css_pattern *sz_part,
                                    const float *prior_x, const float *prior_y, const float *prior_z, int64_t max_iters,
                                    const ldpc_stab_minsum_options *options, ldpc_stab_minsum_decoder **out);
ldpc_status ldpc_stab_minsum_destroy(ldpc_stab_minsum_decoder *dec);
int32_t ldpc_stab_minsum_kernel(const ldpc_stab_minsum_decoder *dec);
int32_t ldpc_stab_minsum_tile_syndromes(const ldpc_stab_minsum_decoder *dec);
int32_t ldpc_stab_minsum_last_grid(const ldpc_stab_minsum_decoder *dec);
ldpc_status ldpc_stab_minsum_decode_batch(ldpc_stab_minsum_decoder *dec, int64_t batch, const uint8_t *syndromes, uint8_t *gx,
                                          uint8_t *gz, uint8_t *converged, double *llr, int32_t *iters);
ldpc_status ldpc_stab_minsum_decode_batch_device(ldpc_stab_minsum_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                                 uint8_t *d_gx, uint8_t *d_gz, uint8_t *d_converged, double *d_llr,
                                                 int32_t *d_iters, void *stream);

#endif /* LDPC_MI355X_STAB_H */
