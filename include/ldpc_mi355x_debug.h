/*
 * ldpc_mi355x_debug.h -- test hooks of libldpc_mi355x.so.  NOT part of the drop-in boundary (include/ldpc_mi355x.h):
 * nothing here replaces a reference interface; the CPU test-suite uses these entries to check, without a GPU, the
 * host-side planning the team kernel relies on (ldpcdecoders.jl_amd/csrc/team_plan.cpp: team_plan_pure(),
 * team_rows_tables(), team_irr_tables()) and the tier / tile-width choice of the min-sum and relay decoders
 * (csrc/tile_plan.hpp) and the layers of the layered min-sum schedule (csrc/layer_plan.hpp).  Pure host code; no device
 * is needed or touched.  Likewise the kernel, tile width and register buckets of the BP-OTS decoder (csrc/bpots_plan.hpp), and
 * how a BP-OTS handle launched its last batch (host fields of the handle).
 */
#ifndef LDPC_MI355X_DEBUG_H
#define LDPC_MI355X_DEBUG_H

#include "ldpc_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How a batch of `batch` syndromes of a graph with nnz edges would be dealt to teams of workgroups on an MI355X
   (256 CUs, one team workgroup per CU, members of >= 2048 message rows) under a budget of cache_mib MiB of message
   slots in flight (the library's default: 240).  rows_dv: the bit degree when the graph is regular and has a
   rows-on-chip instantiation, else 0 (with it the plan counts on 312 rows in LDS and 8 x 32 in registers per member).  out = { members per team (1 = no teams: node-parallel or tile kernel),
   teams = message slots in flight, workgroups launched, XCDs that host teams, 1 if the members of a team are dealt
   over all XCDs (<= 3 tiles), 1 if members keep rows in LDS }. */
ldpc_status ldpc_debug_team_plan(int64_t nnz, int64_t max_iters, int64_t batch, int32_t cache_mib, int32_t rows_dv,
                                 int32_t out[6]);

/* The tables with which the team kernel keeps message rows ON CHIP -- in the members' LDS and in the registers of
   their waves -- for a REGULAR graph (every check dc edges, every bit dv) whose degree pair has an instantiation --
   check degree 6 ... 10 x bit degree 3 ... 5; LDPC_ERR_UNSUPPORTED otherwise -- and teams of `members` workgroups of 8 waves.
   In: regs_per_wave (0 ... 32) rows a wave may keep in registers; static_quarters (0 ... 4): the share of a member's
   chunks per sweep that its waves own by right (only edges between such chunks of ONE wave can live in its registers).
   Out: degrees = {dc, dv}; shape = {words per position record (8 or 16), R = LDS rows per member (at most 312),
   static check chunks, static position chunks per member, register rows per wave in effect};
   vtab [n][shape[0]] = per position of the dealt bit order the CSR rows of its dv edges (row = dc * check + place among
   the check's bits), where each lives (>= 0: that LDS row of the member; -1: the team's slot; <= -2: register row
   -2 - x of the wave), the bit (| 1 << 31 when one of its edges is not in the slot), padding; ctab [s][4] = per check
   the mask of its edges in LDS, the LDS row of the first of them, the mask of its edges in registers, the register
   row of the first of them; lds_edge [members][R] and reg_edge [members][8][regs_per_wave] = the CSR rows held, -1
   beyond the count (pass room for members * 312 and members * 8 * 32).
   No reference counterpart: the reference keeps every message in one dense matrix (belief_propagation.jl:83-91). */
ldpc_status ldpc_debug_team_rows(int64_t s, int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t members,
                                 int32_t regs_per_wave, int32_t static_quarters, int32_t *degrees, int32_t *shape,
                                 int32_t *vtab, int32_t *ctab, int32_t *lds_edge, int32_t *reg_edge);

/* The tables with which the team kernel keeps WHOLE CHECKS of an IRREGULAR graph (any CSC pattern) in the LDS of their
   owners (csrc/team_plan.cpp team_irr_tables(); bp_team_kernels.hpp, IRR), for teams of `members` workgroups and nodes
   inside the register buckets dc_bucket / dv_bucket.  Out: shape = {R = LDS rows per member (at most 312), rows in LDS in
   all}; ctab2 [s + 1][2] = per check {its first CSR row, its first LDS row or -1}; ptab [n + 1][2] = per position of the
   dealt bit order {first entry of its edge list in ploc, the bit | 1 << 31 when one of its edges is in LDS}; ploc [nnz] =
   per edge of a position (checks ascending) its CSR row, or -1 - (LDS row); lds_edge [members][R] (pass room for
   members * 312) = the CSR rows held, -1 beyond a member's count; posmap [n] = the position of every bit.
   No reference counterpart. */
ldpc_status ldpc_debug_team_irr(int64_t s, int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t members,
                                int32_t dc_bucket, int32_t dv_bucket, int32_t *shape, int32_t *ctab2, int32_t *ptab, int32_t *ploc,
                                int32_t *lds_edge, int32_t *posmap);

/* The tier and the tile width ldpc_minsum_create (relay = 0) / ldpc_relay_create (relay != 0) choose for a graph of s
   checks and n bits whose check records take rec_words words (4 per check of degree 1 ... 32, 5 up to 64, the degree
   beyond; 0 for an empty check) -- csrc/tile_plan.hpp tile_plan(), the function both call.  A tile of S syndromes has a
   state of  S (4 (n + rec_words) + s)  bytes (min-sum) or  S (4 (2 n + rec_words + ceil(n / 32)) + s)  bytes (relay),
   rounded up to 256.  tier 1 (on-chip) with the largest power of two S <= 64 whose state fits 79 KiB (two workgroups a
   CU), else the largest that fits 159 KiB; else tier 2 (unlimited) with S = 64.  kernel_variant 1 / 2 force a tier (2:
   S = 64 always; 1 where not even S = 1 fits 159 KiB: LDPC_ERR_UNSUPPORTED, as create answers); 0 = by size.  Out (each
   may be NULL): the tier, S, and the bytes of the state of one tile.  Negative sizes, sizes create refuses and a
   kernel_variant outside 0 .. 2: LDPC_ERR_INVALID_ARGUMENT.  No reference counterpart. */
ldpc_status ldpc_debug_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t relay, int32_t kernel_variant, int32_t *tier,
                                 int32_t *tile_syndromes, int64_t *state_bytes);

/* The second plan of a min-sum handle, for the entries with per-syndrome priors (ldpc_minsum_decode_batch_priors*,
   ldpc_minsum_decode_batch_given*) -- csrc/tile_plan.hpp priors_tile_plan(), the function ldpc_minsum_create calls.
   schedule 0 (flooding): a tile keeps its priors as a fourth block [n][S] f32, so its state is
   round4(S (4 (n + rec_words) + s)) + 4 n S  bytes, rounded up to 256, and the policy of ldpc_debug_tile_plan runs over
   that size.  schedule 1 (layered): no such block; the answer is ldpc_debug_tile_plan's with relay = 0.  Out and
   statuses as there; a schedule outside 0 .. 1: LDPC_ERR_INVALID_ARGUMENT.  No reference counterpart. */
ldpc_status ldpc_debug_priors_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t schedule, int32_t kernel_variant,
                                        int32_t *tier, int32_t *tile_syndromes, int64_t *state_bytes);

/* The plan of a joint X/Z (Pauli) min-sum handle -- csrc/tile_plan.hpp pauli_tile_plan(), the function
   ldpc_pauli_minsum_create calls.  s = rx + rz checks of both sides, n qubits, rec_words over the checks of both sides
   (counted as for ldpc_debug_tile_plan).  A tile of S syndromes has a state of  S (4 (2 n + rec_words) + s)  bytes,
   rounded up to 256, and the policy of ldpc_debug_tile_plan runs over that size.  Out and statuses as there.  No
   reference counterpart. */
ldpc_status ldpc_debug_pauli_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                       int32_t *tile_syndromes, int64_t *state_bytes);

/* The plan of a guided-decimation min-sum handle -- csrc/tile_plan.hpp decim_tile_plan(), the function
   ldpc_decim_create calls.  A tile of S syndromes has a state of  S (4 (n + rec_words + ceil(n / 32)) + s)  bytes (L, the
   check records, a bit per decimated bit, the syndromes), rounded up to 256, and the policy of ldpc_debug_tile_plan runs
   over that size.  Out and statuses as there.  No reference counterpart. */
#include "ldpc_mi355x_decim_debug.h"   /* (declares it: this header keeps the hooks it declared before) */

/* The plan of a Pauli relay min-sum handle -- csrc/tile_plan.hpp pauli_relay_tile_plan(), the function
   ldpc_pauli_relay_create calls; s = rx + rz and rec_words count the checks of both sides.  A tile of S syndromes has a
   state of  S (4 (6 n + rec_words + 2 ceil(n / 32)) + s)  bytes (the three beliefs the check sweep reads, the three
   posteriors, the check records, a bit plane each for the X part and the Z part of the lightest solution, the syndromes),
   rounded up to 256, and the policy of ldpc_debug_tile_plan runs over that size.  Out and statuses as there.  No reference
   counterpart. */
#include "ldpc_mi355x_pauli_relay_debug.h"   /* (declares ldpc_debug_pauli_relay_tile_plan) */

/* The plan of a stabilizer min-sum handle -- csrc/tile_plan.hpp stab_tile_plan(), the function ldpc_stab_minsum_create
   calls; r checks, n qubits, rec_words over the checks of the union graph.  A tile of S syndromes has a state of
   S (4 (3 n + rec_words) + r)  bytes (the three message totals MX, MY, MZ, the check records, the syndromes), rounded up to
   256, and the policy of ldpc_debug_tile_plan runs over that size.  Out and statuses as there.  No reference counterpart. */
#include "ldpc_mi355x_stab_debug.h"   /* (declares ldpc_debug_stab_tile_plan) */

/* The layers ldpc_minsum_create gives a handle of the layered schedule (options->schedule = 1; THE LAYERED RULE of
   include/ldpc_mi355x.h) -- csrc/layer_plan.hpp layer_plan_build(), the function create calls, followed by the same
   verification (no two checks of a layer share a bit, every non-empty check in exactly one layer).  H as the zero-based
   CSC pattern create takes.  Out (each may be NULL): layer_of [s] = the layer of every check, -1 for a check with no
   bits; K = the number of layers (0 for a graph without edges).  A pattern create refuses: LDPC_ERR_INVALID_ARGUMENT.
   No reference counterpart. */
ldpc_status ldpc_debug_layer_plan(int64_t s, int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t *layer_of,
                                  int32_t *K);

/* The kernel ldpc_bpots_create chooses for a graph of s checks, n bits and nnz edges whose largest check has max_cdeg
   edges and whose largest bit has max_bdeg -- csrc/bpots_plan.hpp ots_plan(), the function create calls.  A workgroup of
   the LDS-resident kernel that decodes S syndromes at a time keeps
       8 S nnz + 12 S n + 24 n + 32 s + 2112 + 24 * 512 + 2 (s + n + 2 + 2 nnz) + 32
   bytes in dynamic LDS.  Kernel 2 (LDS-resident) with the largest S = 1 ... 64 for which that plus 8192 fits 76 KiB; else
   with S = 1 where that fits 156 KiB (the large budget is only ever taken with S = 1).  Never for s, n or nnz >= 65535, a
   check of more than 32 or a bit of more than 16 edges (`wide`), or force_node != 0 (what LDPC_BPOTS_FORCE_NODE sets in
   the experiments build).  Else kernel 3 (node-parallel; LDS: round16(s + 3 n) + 4 s + 28 * 1024 + 64 bytes), unless the
   graph is wide, force_node >= 2 or that plus 1024 is past 156 KiB: kernel 5 (unlimited, no dynamic LDS).  Out (each may be
   NULL): the kernel as ldpc_bpots_kernel reports it; log2 S (-1 outside kernel 2); the dynamic LDS bytes of the choice;
   the budget it fits in KiB (76 or 156; 0 outside kernel 2); the register buckets of the instantiation, dc = 8 or 32 and
   dv = 4 or 16 (0 for kernel 5).  A negative argument: LDPC_ERR_INVALID_ARGUMENT; s, n or nnz >= 2^28: LDPC_ERR_UNSUPPORTED,
   as create answers.  No reference counterpart. */
ldpc_status ldpc_debug_bpots_plan(int64_t s, int64_t n, int64_t nnz, int32_t max_cdeg, int32_t max_bdeg, int32_t force_node,
                                  int32_t *kernel, int32_t *logS, int64_t *lds_bytes, int32_t *budget_kib, int32_t *dc, int32_t *dv);

/* How the most recent decode of a BP-OTS handle was launched; reads host fields of the handle only.  Out (each may be
   NULL): path 0 = nothing launched (no decode yet, or max_iters == 0), 1 = the latency path of the host entry (one
   workgroup per group, results through a host-mapped image), 2 = workgroups that take groups from a queue; groups = tiles
   of S syndromes (kernel 2) or syndromes (kernels 3, 5) of the batch; the workgroups launched; chunk = groups a workgroup
   takes from the queue at a time; per_cu = workgroups a CU holds as the occupancy query answered (kernel 2; else 0). */
ldpc_status ldpc_debug_bpots_last_launch(const ldpc_bpots_decoder *dec, int32_t *path, int64_t *groups, int32_t *grid,
                                         int32_t *chunk, int32_t *per_cu);

/* Two builds of the library in one process (the product and the -DLDPC_EXPERIMENTS build: the Python host of the tests)
   must not run team grids on one device at the same time -- every member of a team has to be resident.  Each build
   orders its own team launches through a per-device event table; the build loaded second adopts the table of the
   first: adopt(process_state of the other build).  Call before the adopting build has launched anything. */
void *ldpc_debug_process_state(void);
ldpc_status ldpc_debug_adopt_process_state(void *state);

/* The one entry here that needs the GPU: out_core[i] = div_core(num[i], den[i]) -- the nine instructions in the middle of
   hipcc's IEEE double division, which the check sweep runs alone where a wave's operands rule the end cases out
   (bp_kernels.hpp, LDPC_FAST_DIV) -- and out_ieee[i] = num[i] / den[i], computed on the device from HOST arrays of
   `count` doubles each.  A GPU test holds the two against each other over the ranges the kernels take the short form
   in, edges included.  No reference counterpart (Julia's `/` is the IEEE division). */
ldpc_status ldpc_debug_div_check(int64_t count, const double *num, const double *den, double *out_core, double *out_ieee);

/* ... and one more: out_fast[i] = the LLR every kernel of the library returns for posterior odds odds[i] (bp_kernels.hpp
   llr_of without llr_exact: the odds cut to their upper 32 bits, then llr_cut -- frexp, one division, seven terms of
   2 atanh), out_lib[i] = the library's log(1 / .) of the same cut odds; HOST arrays of `count` doubles.  A GPU test holds
   them against each other (<= 1e-12, end cases identical) and against log(1 / odds) (<= 5e-7).  Reference:
   belief_propagation.jl:163. */
ldpc_status ldpc_debug_llr_check(int64_t count, const double *odds, double *out_fast, double *out_lib);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_MI355X_DEBUG_H */
