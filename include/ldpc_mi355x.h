/*
 * ldpc_mi355x.h -- C ABI of libldpc_mi355x.so, the MI355X (gfx950) drop-in for
 * the belief-propagation hot path of QuantumSavory/LDPCDecoders.jl.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference checkout).  The reference has no FFI of its own (it is pure
 * Julia); these are the symbols a `ccall` shim binds -- see INTEGRATION.md and
 * ldpcdecoders.jl_amd/julia/LDPCDecodersMI355X.jl.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross the boundary: every
 *     call returns an ldpc_status and ldpc_last_error() holds the message of
 *     the last failure on the calling thread.
 *   - a handle is NOT re-entrant (neither is the reference decoder, whose
 *     scratch is shared: belief_propagation.jl:58); different handles may be
 *     used from different threads.
 *   - batch layout is the memory image of the reference's column-major Julia
 *     matrices: syndromes (s x B) = B contiguous runs of s bytes; errors
 *     (n x B) = B contiguous runs of n bytes.
 *   - the library never keeps a caller pointer after a call returns.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry returns LDPC_ERR_NO_DEVICE.
 */
#ifndef LDPC_MI355X_H
#define LDPC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_MI355X_ABI_VERSION 4

typedef enum ldpc_status {
    LDPC_OK = 0,
    LDPC_ERR_INVALID_ARGUMENT = 1, /* shape / pointer / CSC-pattern errors (reference: AssertionError, BoundsError) */
    LDPC_ERR_NO_DEVICE = 2,        /* no gfx950 device or HIP runtime unusable */
    LDPC_ERR_HIP = 3,              /* a HIP call failed; text in ldpc_last_error() */
    LDPC_ERR_OUT_OF_MEMORY = 4,
    LDPC_ERR_UNSUPPORTED = 5
} ldpc_status;

typedef struct ldpc_bp_decoder ldpc_bp_decoder; /* opaque; owns device copies of H and the workspace */

/* Sizes and tuning of a decoder, readable after create.
 * Mirrors the public fields of `BeliefPropagationDecoder`
 * (src/decoders/belief_propagation.jl:38-59: per, max_iters, s, n). */
typedef struct ldpc_bp_info {
    int64_t s, n, nnz;
    int64_t max_iters;
    double per;
    int32_t max_check_degree, max_bit_degree;
    int32_t device;           /* HIP device ordinal */
    int32_t tile_syndromes;   /* syndromes decoded together by one workgroup (lane = syndrome) */
    int32_t waves_per_tile;   /* wavefronts cooperating on one tile */
    int32_t resident_tiles;   /* workgroups in the persistent grid of the most recent batch call (tile kernel: one
                                 message slot each; team kernel: last_team_size per message slot) */
    int64_t workspace_bytes;  /* device bytes held by the handle */
    int32_t last_kernel;      /* kernel the most recent batch call ran: 0 none yet, 1 HBM-streaming tile kernel,
                                 2 LDS-resident, 3 node-parallel, 4 team (numbered like kernel_variant) */
    int32_t last_team_size;   /* workgroups per tile of that call (1 unless last_kernel == 4) */
    int32_t last_lds_rows;    /* team kernel: message rows each member kept in its LDS in that call (0 = every row in the
                                 team's slot; regular graphs with a rows-in-LDS instantiation keep up to 312) */
    int32_t last_rows_on_chip;/* team kernel: message rows of a tile (of its nnz) that lived in the members' LDS and in their
                                 waves' registers in that call and never touched the team's slot */
    int32_t reserved_info[2];
} ldpc_bp_info;

/* Optional knobs; pass NULL to ldpc_bp_create for defaults.  Zero = default. */
typedef struct ldpc_bp_options {
    int32_t device;           /* HIP device ordinal; -1 = current device */
    int32_t waves_per_tile;   /* 0 = auto (8; 16 when the batch has at most one tile per CU); else 4, 8, 16 */
    int32_t resident_tiles;   /* 0 = auto (fills the chip) */
    int32_t kernel_variant;   /* 0 = auto: LDS-resident kernel when the edge messages of >= 1 syndromes, the masks and
                                 the graph fit a CU's LDS; node-parallel kernel (one workgroup per syndrome) when
                                 only ONE syndrome's messages fit it, at every batch size; beyond that a cost
                                 model picks between the node-parallel kernel and the team kernel (several
                                 workgroups per 64-syndrome tile) for small batches; the team kernel takes the larger
                                 ones with PERSISTENT teams (a team decodes tile after tile in its own message slot)
                                 when a chip-wide set of slots fits the 256 MiB Infinity Cache or is at most 3.3 x
                                 the 240 MiB budget planned for it (n <= 49152 for (4,8)-regular codes), else with one
                                 team per tile up to one tile per CU; the
                                 HBM-streaming tile kernel (one persistent workgroup per tile) takes the rest.
                                 1 = force streaming; 2 = force LDS-resident (error if it does not fit);
                                 3 = force node-parallel; 4 = team kernel wherever it applies, streaming otherwise
                                 (never LDS-resident / node-parallel).
                                 ldpc_bp_info.last_kernel reports what ran */
    int32_t defer_threshold;  /* HBM-streaming kernel: a 64-syndrome tile hands its unconverged syndromes to a
                                 densely packed second pass once at most this many are left (same results,
                                 fewer nearly-empty sweeps).  0 = auto (16), -1 = off, else 1..48 */
    int32_t llr_exact;        /* What `llr` holds.  0 (default): log(1 / T~), T~ = the posterior odds T of :163 cut to their upper
                                 32 bits (20 fraction bits) -- the same bits whatever kernel finishes a syndrome, within
                                 5e-7 of the reference's log(1 / T) (2e-6 where T is denormal, LLR > 708.39; BASELINE.json asks
                                 for 1e-5); +-Inf come out exactly.
                                 The team kernel of large codes then captures 4 bytes per bit and iteration instead of 8
                                 (LLRs at the C3 size: +5 % kernel time at 50 iterations instead of +19 %).  1: log(1 / T) of T itself, as
                                 before ABI version 4 -- what the BP+OSD hosts ask for, because OSD orders the bits by
                                 reliability (belief_propagation_osd.jl:53-55) and two reliabilities that differ in the
                                 21st bit must not become a tie.  Hard decisions, flags and iteration counts do not
                                 depend on it */
    int32_t reserved[10];
} ldpc_bp_options;

/* Library / ABI version and build target ("gfx950"). */
int32_t ldpc_abi_version(void);
const char *ldpc_build_target(void);

/* Message of the last failed call on this thread ("" if none). */
const char *ldpc_last_error(void);

/* The message arrays of large codes (>= 1 GiB) are groups of 1 GiB chunks that the library keeps, still mapped, in a
 * per-process pool when a decoder lets go of them, so that the next decoder of that size takes them over (at most
 * 64 GiB are held; the pool is emptied by itself when an allocation runs out of memory).  This gives
 * everything in the pool back to the device now; decoders in use are not affected. */
ldpc_status ldpc_trim_memory(void);

/* Number of usable gfx950 devices (0 when there is none; never fails). */
int32_t ldpc_device_count(void);

/* Every wait of the HOST for the device inside this library (event / stream / device synchronisation, the flag spin of
 * the single-decode latency path, the synchronisation in front of a free) is bounded: when the device has not got there
 * after this many milliseconds the call returns LDPC_ERR_HIP, ldpc_last_error() names the wait, the device is taken to
 * be stalled for the rest of the process (every later call on it fails at once with the same message, nothing it may
 * still use is freed).  Per process; default 600000 (ten minutes: longer than any single call on the configurations of
 * BASELINE.json by two orders of magnitude); 0 = wait for ever (the behaviour before ABI version 4).  The reference has no
 * counterpart (pure host code).  Device-side waits have bounds of their own (team barrier 10 s, roll call 20 ms). */
ldpc_status ldpc_set_wait_limit_ms(int64_t ms);
int64_t ldpc_get_wait_limit_ms(void);

/*
 * Replaces `BeliefPropagationDecoder(H, per::Float64, max_iters::Int)`
 * (src/decoders/belief_propagation.jl:61-67) together with the scratch
 * constructor (:20-22).
 *
 * H arrives as the CSC pattern that `sparse(H)` builds at :63 -- colptr[n+1],
 * rowval[nnz], ZERO-based, row indices strictly ascending inside each column
 * (Julia's SparseMatrixCSC invariant; the message products depend on that
 * order).  Every stored entry is an edge, as in the reference, which walks
 * `nzrange` without looking at the stored Bool (:128,137,155).  The transpose
 * pattern (`sparse(H')`, :64) is derived inside.
 */
ldpc_status ldpc_bp_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr,
                           const int64_t *rowval, double per, int64_t max_iters,
                           const ldpc_bp_options *options, ldpc_bp_decoder **out);

/* Frees device memory and the handle (the reference relies on Julia's GC). */
ldpc_status ldpc_bp_destroy(ldpc_bp_decoder *dec);

ldpc_status ldpc_bp_get_info(const ldpc_bp_decoder *dec, ldpc_bp_info *info);

/*
 * Replaces `batchdecode!(decoder, syndromes, errors, success)`
 * (src/decoders/belief_propagation.jl:220-231; 3-argument form
 * src/decoders/abstract_decoder.jl:44-48) and, with batch = 1,
 * `decode!(decoder, syndrome)` (:121-188) including its leading `reset!`
 * (:83-91, :122).  HOST buffers.
 *
 *   syndromes [batch][s] uint8   in : entry parity gives the sign (-1)^x (:136); an entry
 *                                     other than 0/1 can never satisfy the convergence `==` (:181)
 *   errors    [batch][n] uint8   out: hard decisions 0/1 of the last executed iteration (:164-168)
 *   converged [batch]    uint8   out: 1 iff the syndrome was matched within max_iters (:180-184)
 *   llr       [batch][n] double  out, may be NULL: scratch.log_probabs = log(1/temp) (:163)
 *   iters     [batch]    int32   out, may be NULL: iterations executed (extension; reference has none)
 *
 * max_iters = 0 yields zeros / converged = 0 / llr = 0 exactly like the reference.
 */
ldpc_status ldpc_bp_decode_batch(ldpc_bp_decoder *dec, int64_t batch, const uint8_t *syndromes,
                                 uint8_t *errors, uint8_t *converged, double *llr, int32_t *iters);

/*
 * Same contract with DEVICE pointers (HBM-resident batches: the multi-GPU
 * shards of INTEGRATION.md, and bench.py).  Work is enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream) and is
 * asynchronous; outputs are valid once the stream has been synchronised.
 * Calls on one handle share its workspace and therefore execute in call
 * order: a call given another stream than its predecessor waits (on the
 * device) for that predecessor first.  ldpc_bp_last_status() tells whether
 * the asynchronous work went well.
 */
ldpc_status ldpc_bp_decode_batch_device(ldpc_bp_decoder *dec, int64_t batch,
                                        const uint8_t *d_syndromes, uint8_t *d_errors,
                                        uint8_t *d_converged, double *d_llr, int32_t *d_iters,
                                        void *stream);

/*
 * The same `batchdecode!(decoder, syndromes, errors, success)` (src/decoders/belief_propagation.jl:220-231) on
 * BIT-PACKED matrices in the memory layout of a Julia `BitMatrix` -- what the reference's own test and doctest hand in
 * as `errors` (test/test_bp_decoder.jl:26, belief_propagation.jl:217).  A BitMatrix of r x B keeps element (row, col),
 * zero-based, as bit k = col * r + row of one flat bit string: word k >> 6 of `chunks::Vector{UInt64}`, bit k & 63,
 * least significant bit first, columns NOT padded.  HOST buffers.
 *
 *   syndrome_words  uint64, 8-byte aligned, little-endian   in : the syndrome bit of (check r, column i) is bit
 *                                                                syndrome_bit0 + i * s + r
 *   error_words     uint64, 8-byte aligned, little-endian   out: the error bit of (bit j, column i) is bit
 *                                                                error_bit0 + i * n + j
 *   syndrome_bit0, error_bit0 >= 0: 0 for a whole BitMatrix; c0 * r addresses column c0 onward of a larger one
 *   converged [batch] uint8, llr [batch][n] double (may be NULL), iters [batch] int32 (may be NULL): exactly as in
 *   ldpc_bp_decode_batch (a Julia Vector{Bool} is a byte per element already)
 *
 * The call writes EXACTLY the bits [error_bit0, error_bit0 + batch * n): every other bit of the first and the last
 * word it touches keeps its value (a BitMatrix keeps its trailing bits zero; a view does not damage its neighbours),
 * words wholly inside the range are overwritten.  Only the words that cover a range are read or written.
 * Hard decisions, flags, iteration counts and LLRs are those of ldpc_bp_decode_batch on the same syndromes, bit for
 * bit: the same kernels under the same plan run on a byte image that the handle owns (counted in workspace_bytes); two
 * streaming kernels convert at the boundary.  batch = 0: LDPC_OK, nothing touched.  max_iters = 0: the range becomes
 * zeros.  s = 0 / n = 0 as in the byte entry.  A NULL handle, a negative batch or bit offset, a word pointer that is
 * not 8-byte aligned, a NULL pointer where the byte entry rejects one: LDPC_ERR_INVALID_ARGUMENT before any device work.
 *
 * These three entries were added WITHOUT a change of LDPC_MI355X_ABI_VERSION (they only add symbols): a caller detects
 * them by symbol lookup (dlsym / Libdl.dlsym).
 */
ldpc_status ldpc_bp_decode_batch_bits(ldpc_bp_decoder *dec, int64_t batch, const uint64_t *syndrome_words,
                                      int64_t syndrome_bit0, uint64_t *error_words, int64_t error_bit0,
                                      uint8_t *converged, double *llr, int32_t *iters);

/*
 * The bits entry with DEVICE pointers: asynchronous on `stream` and ordered on the handle exactly like
 * ldpc_bp_decode_batch_device (bits -> bytes, that entry's kernels, bytes -> bits, all on `stream`).
 * ldpc_bp_last_status / ldpc_bp_last_timing cover it; total_ms includes the two conversions.  The partial first / last
 * word of the error range is read, merged and written back by the call: nothing else may write those two words
 * until the call has finished.
 */
ldpc_status ldpc_bp_decode_batch_bits_device(ldpc_bp_decoder *dec, int64_t batch, const uint64_t *d_syndrome_words,
                                             int64_t syndrome_bit0, uint64_t *d_error_words, int64_t error_bit0,
                                             uint8_t *d_converged, double *d_llr, int32_t *d_iters, void *stream);

/*
 * Was everything enqueued on this handle so far good?  Waits for the most recent
 * ldpc_bp_decode_batch_device call (and with it every earlier one: calls on a handle run in call
 * order, whatever streams they were given) and returns LDPC_OK, or LDPC_ERR_HIP if a team of
 * workgroups lost a member during one of them (a team barrier timed out after ~10 s; the team
 * kernel serves medium batches on large codes).  ldpc_last_error() then names the first call hit;
 * the outputs of that call and of every team-kernel call enqueued after it are invalid and must be
 * decoded again -- the decoder keeps teams off from then on, so the retry cannot fail the same way.
 * The fault is reported exactly once: by this function, or by the next
 * ldpc_bp_decode_batch_device call on the handle (which then enqueues nothing), whichever comes
 * first.  The host-buffer entry ldpc_bp_decode_batch is synchronous and repairs such a call itself.
 */
ldpc_status ldpc_bp_last_status(ldpc_bp_decoder *dec);

/*
 * Timing of the most recent ldpc_bp_decode_batch[_device] call, taken with HIP
 * events on the stream the kernels were launched on.  Blocks until that call
 * has finished.  sweep_ms = the message-passing kernel alone (the roofline
 * kernel), total_ms = pack + sweeps + unpack.  sum_iters = sum over the batch
 * of iterations executed (the factor of the algorithmic byte count,
 * 32 * nnz bytes per syndrome * iteration).
 */
ldpc_status ldpc_bp_last_timing(ldpc_bp_decoder *dec, double *sweep_ms, double *total_ms,
                                int64_t *sum_iters);

/* Same for an earlier call: calls_back = 0 is the most recent batch call, 1 the
 * one before, ... up to 15 (a ring of 16 event sets).  Lets a caller time K
 * back-to-back asynchronous calls without synchronising between them. */
ldpc_status ldpc_bp_call_timing(ldpc_bp_decoder *dec, int32_t calls_back, double *sweep_ms,
                                double *total_ms, int64_t *sum_iters);

/* ------------------------------------------------------------------------
 * batchdecode! over several GPUs of one node from ONE process (BASELINE config 4).
 *
 * `batchdecode!(decoder, syndromes, errors, success)` (src/decoders/belief_propagation.jl:220-231) is one call on one
 * caller-held s x B matrix whose columns are decoded independently (:224-228).  A multi-device decoder keeps that
 * contract: logical device g decodes the contiguous columns [g*B/G, (g+1)*B/G) with a single-device handle of its own
 * (its own copy of the Tanner graph, workspace and stream); there is no collective inside the decode.  This is what a
 * Julia host binds with `ccall`; a host that runs one process per GPU (PyTorch) shards the same way
 * above the single-device entries instead (ldpcdecoders.jl_amd/sharding.py).
 * ------------------------------------------------------------------------ */
#define LDPC_MULTI_MAX_DEVICES 16

/* How the ROOT-DEVICE form moves shards between devices[0] and the others. */
enum {
    LDPC_EXCHANGE_AUTO = 0, /* create: RCCL when every logical device is a GPU of its own, else COPY; one device: NONE */
    LDPC_EXCHANGE_COPY = 1, /* hipMemcpyPeerAsync ordered by events (logical devices that share a GPU cannot form an RCCL
                               clique: the rehearsal of G shards on fewer GPUs) */
    LDPC_EXCHANGE_RCCL = 2, /* one RCCL communicator per device (ncclCommInitAll, created by the first root-device call);
                               scatter and gather are ncclGroupStart / ncclSend + ncclRecv / ncclGroupEnd over xGMI.  RCCL
                               is loaded at run time (librccl.so.1).  With ONE device the shard travels to itself through a
                               one-rank communicator (a rehearsal of the RCCL calls on a one-GPU box) */
    LDPC_EXCHANGE_NONE = 3  /* (reported only) one device: the batch is decoded where it lies */
};

typedef struct ldpc_bp_multi ldpc_bp_multi; /* opaque; owns one ldpc_bp_decoder, one stream and the shard buffers per device */

typedef struct ldpc_bp_multi_info {
    int32_t ndev;
    int32_t exchange;                         /* LDPC_EXCHANGE_NONE / _COPY / _RCCL */
    int32_t devices[LDPC_MULTI_MAX_DEVICES];  /* HIP ordinal of logical device g; g = 0 is the root */
    /* the most recent ldpc_bp_decode_batch_multi_device call, from HIP events on the root's stream (zeros after a
       host-form call): */
    double scatter_ms;      /* enqueueing + sending the syndrome shards */
    double root_decode_ms;  /* the root's own shard */
    double gather_ms;       /* receiving the results: includes waiting for the slowest peer's decode */
    double decode_ms_max;   /* slowest device's pack + sweeps + unpack (its handle's ldpc_bp_last_timing) */
    int64_t scatter_bytes_per_peer, gather_bytes_per_peer;
} ldpc_bp_multi_info;

/* The constructor of ldpc_bp_create (belief_propagation.jl:61-67), once per logical device: devices[ndev] are HIP
 * ordinals (an ordinal may appear more than once: those logical devices share the GPU and their team grids run one
 * after the other), devices[0] is the root of the root-device form.  options->device is ignored. */
ldpc_status ldpc_bp_create_multi(int32_t ndev, const int32_t *devices, int32_t exchange, int64_t s, int64_t n, int64_t nnz,
                                 const int64_t *colptr, const int64_t *rowval, double per, int64_t max_iters,
                                 const ldpc_bp_options *options, ldpc_bp_multi **out);
ldpc_status ldpc_bp_destroy_multi(ldpc_bp_multi *dec);

/* The single-device handle of logical device g (ldpc_bp_get_info, ldpc_bp_call_timing ...); NULL if out of range.
 * Owned by the multi-device decoder: do not destroy it, and do not decode through it while a multi call is in flight. */
ldpc_bp_decoder *ldpc_bp_multi_handle(ldpc_bp_multi *dec, int32_t g);

/* `batchdecode!` (belief_propagation.jl:220-231) on HOST buffers laid out as for ldpc_bp_decode_batch: shard g goes
 * pinned host -> ITS OWN GPU -> pinned host through that device's 3-slot copy / decode / copy pipeline, one host thread
 * per device; nothing hops through GPU 0.  Synchronous.  With ndev = 1 this is ldpc_bp_decode_batch. */
ldpc_status ldpc_bp_decode_batch_multi(ldpc_bp_multi *dec, int64_t batch, const uint8_t *syndromes, uint8_t *errors,
                                       uint8_t *converged, double *llr, int32_t *iters);

/* ldpc_bp_decode_batch_bits (the BitMatrix layout, belief_propagation.jl:220-231) over the devices, HOST buffers: device g
 * takes the columns [g*B/G, (g+1)*B/G) through the single-device bits entry with syndrome_bit0 + lo * s and
 * error_bit0 + lo * n.  Shard borders do not fall on words: two shards may share an error word, and each merges its bits
 * into it with atomic operations on the word.  Synchronous.  There is no root-device form in bits. */
ldpc_status ldpc_bp_decode_batch_multi_bits(ldpc_bp_multi *dec, int64_t batch, const uint64_t *syndrome_words,
                                            int64_t syndrome_bit0, uint64_t *error_words, int64_t error_bit0,
                                            uint8_t *converged, double *llr, int32_t *iters);

/* The same with the whole batch resident in the HBM of devices[0] (pointers as for ldpc_bp_decode_batch_device):
 * scatter the syndrome shards, decode, gather hard decisions / flags (/ iteration counts / LLRs) into the caller's
 * arrays.  Asynchronous: the root's work is enqueued on `stream` (a hipStream_t of devices[0]; NULL = its default
 * stream), the peers' on streams of their own; the outputs are valid once `stream` has been synchronised.  With
 * ndev = 1 (and no RCCL rehearsal) this is ldpc_bp_decode_batch_device. */
ldpc_status ldpc_bp_decode_batch_multi_device(ldpc_bp_multi *dec, int64_t batch, const uint8_t *d_syndromes,
                                              uint8_t *d_errors, uint8_t *d_converged, double *d_llr, int32_t *d_iters,
                                              void *stream);

/* ldpc_bp_last_status over every device: waits for the most recent call everywhere and reports the first failure. */
ldpc_status ldpc_bp_multi_last_status(ldpc_bp_multi *dec);
/* Blocks until the most recent root-device call has finished. */
ldpc_status ldpc_bp_multi_get_info(ldpc_bp_multi *dec, ldpc_bp_multi_info *info);

/* ------------------------------------------------------------------------
 * BP+OSD host post-processing (BASELINE config 5).  Pure host
 * code (bit-packed GF(2) elimination, threaded over the batch): it consumes the
 * BP outputs of ldpc_bp_decode_batch and needs no device.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_osd ldpc_osd;

/* Replaces the OSD half of `BeliefPropagationOSDDecoder(H, per, max_iters; osd_order)`
 * (src/decoders/belief_propagation_osd.jl:17-29): keeps a bit-packed copy of H
 * (zero-based CSC pattern as for ldpc_bp_create) and the OSD order. */
ldpc_status ldpc_osd_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr,
                            const int64_t *rowval, int64_t osd_order, ldpc_osd **out);
ldpc_status ldpc_osd_destroy(ldpc_osd *osd);

/* Replaces lines :52-60 of `decode!(::BeliefPropagationOSDDecoder, syndrome)` and the
 * `osd` methods (:63-125 order 0, :127-209 order > 0) for a batch:
 *   syndromes [batch][s] uint8 (0/1 only), bp_errors [batch][n] uint8 and llr [batch][n]
 *   double = the BP outputs; errors [batch][n] uint8 out.  nthreads <= 0: all host cores. */
ldpc_status ldpc_osd_postprocess_batch(const ldpc_osd *osd, int64_t batch, const uint8_t *syndromes,
                                       const uint8_t *bp_errors, const double *llr, uint8_t *errors,
                                       int32_t nthreads);

/* The same step ON THE DEVICE, opt-in (the host form above stays the default): new HIP kernels for gfx950
 * (csrc/osd_kernels.hpp), for BP outputs that are already device-resident.
 *
 * The rule, stated because two libms do not return the same ulp of exp: p = pm_exp(llr) (csrc/portable_math.h,
 * bit-identical on host and device), key = p > 1-p ? p : 1-p, columns ordered by (key descending, column index
 * ascending).  A NaN LLR (BP produces none for 0 < per < 1) orders last among all columns, by ascending index.  On the
 * rare syndrome where libm's exp and pm_exp (<= 1 ulp apart) order two nearly tied columns differently, the device form
 * may return another, equally valid estimate than the host form.  A syndrome entry that is not 0 counts as 1 (an
 * asynchronous entry cannot return a per-entry status; the host entry's rejection stays).  bp_errors entries are 0 / 1.
 * The estimate for a syndrome outside the column space of H (no error has it) is not specified.
 *
 * ldpc_osd_device_prepare: once per handle.  device = -1: the current device.  Uploads the packed rows, picks the tier
 * (kernel_variant 0) or takes the forced one (1..3; LDPC_ERR_UNSUPPORTED when a syndrome's state does not fit tier 1 /
 * 2), allocates the tier-3 workspace.  osd_order > 16 (2^16 candidates per syndrome): LDPC_ERR_UNSUPPORTED, use the
 * host entry.  Arguments are checked before any device work.
 * ldpc_osd_device_kernel: 1 = on-chip, one wave per syndrome (s <= 128, n <= 512); 2 = on-chip, one 16-wave workgroup
 * per syndrome, working rows in dynamic LDS (state <= 159 KiB: s * 8 * (n/64 + 1 made odd) + 12 n + 4 s + the candidate
 * bitsets; `parity_check_matrix(1000, 10, 9)` takes 138 KiB); 3 = unlimited (state in a slot of a global workspace,
 * grid capped so that the slots stay below 1 GiB); 0 = not prepared / NULL.
 * ldpc_osd_postprocess_batch_device: DEVICE pointers, asynchronous on `stream`, shapes as ldpc_osd_postprocess_batch.
 * d_errors may alias d_bp_errors (in place).  batch = 0: LDPC_OK, nothing touched.  Calls on one handle run in call
 * order whatever streams they are given.  ldpc_osd_destroy frees the device side. */
ldpc_status ldpc_osd_device_prepare(ldpc_osd *osd, int32_t device, int32_t kernel_variant);
int32_t ldpc_osd_device_kernel(const ldpc_osd *osd);
ldpc_status ldpc_osd_postprocess_batch_device(ldpc_osd *osd, int64_t batch, const uint8_t *d_syndromes,
                                              const uint8_t *d_bp_errors, const double *d_llr, uint8_t *d_errors,
                                              void *stream);

/* THE STANDARD RULE, a second rule on the same handle: opt-in, DEVICE FORM ONLY (csrc/osd_search_kernels.hpp).  The rule
 * above is the reference's and stays the default: its key max(exp(llr), 1 - exp(llr)) puts the bits BP is most certain
 * of first.  OSD as published (Panteleev-Kalachev 2021; Roffe et al. 2020) eliminates the columns most likely to be in
 * error first, searches by the combination sweep and weighs a correction by the priors.  Everything below is integer
 * arithmetic or an exact comparison of doubles, so a numpy model equals the device in every element.
 *
 * Per handle: H (s x n); method 1 = exhaustive, 2 = combination sweep; order = lambda >= 0 (at most 16 for method 1,
 * at most 64 for method 2); one weight q[j] (int64) per bit: all 1 (the Hamming weight; channel_llr = NULL), or from
 * channel_llr[n] by the relay decoder's formula, q[j] = (int64) rint(clamp(channel_llr[j], -2^24, 2^24) * 2^16) (ties to
 * even).  Entries must be finite and may be negative.  n <= 2^22, so that a cost fits int64.
 * Per syndrome: syn[s] (an entry that is not 0 counts as 1), bp_err[n] (0 / 1), llr[n] double.
 *   1. If H bp_err == syn the output is bp_err unchanged, at every order.
 *   2. The columns are ordered by ascending llr, the most likely in error first: -0.0 equals +0.0, ties go by ascending
 *      column index, a NaN comes last (after +inf), NaNs among themselves by index.
 *   3. The pivot columns are the greedy independent set in that order, r of them; the non-pivot columns, in that order,
 *      are t_0 ... t_{K-1}, K = n - r.
 *   4. For a set F of non-pivot columns, e(F) is 1 on F, 0 on every other non-pivot column, and has the unique pivot
 *      bits with H e = syn.  The BP hard decisions are not used beyond step 1.  For a syndrome outside the column space
 *      of H the output is not specified.
 *   5. The candidates, with w = min(lambda, K), in a fixed enumeration.  Exhaustive: index x in [0, 2^w), F = {t_k : bit k
 *      of x}.  Combination sweep: index 0, F empty (OSD-0); index 1 + k, F = {t_k}, for EVERY k < K; then F = {t_a, t_b}
 *      for a < b < w, a ascending then b ascending, from index 1 + K on.
 *   6. cost(F) = sum over j of e(F)[j] * q[j] in int64.  The output is the e(F) with the smallest (cost, index).
 *
 * ldpc_osd_set_search(osd, method, order, n, channel_llr_or_NULL): before ldpc_osd_device_prepare; replaces the order
 * given to ldpc_osd_create.  method 0 restores the reference rule (order up to 40, no weights).  LDPC_ERR_INVALID_ARGUMENT
 * for a NULL handle, a method outside 0..2, an order that is negative or beyond its method's bound, an n that is not the
 * handle's, a channel_llr entry that is not finite, weights next to method 0, and a handle that is already prepared;
 * LDPC_ERR_UNSUPPORTED for n > 2^22 with method 1 or 2.  A call that fails changes nothing.
 * ldpc_osd_search_method: the method of the handle (0 for NULL).  ldpc_osd_search_weight(osd, j): q[j] as the handle holds
 * it (1 without weights; 0 for NULL or j outside [0, n)).
 * On such a handle ldpc_osd_device_prepare picks the tier by the state of THIS rule's kernel (tier 1: s <= 128, n <= 512
 * as above; tier 2: s * 8 * (n/64 + 1 made odd) + 16 n + 12 s + 16 (ceil(n/64) + 1) + 520 (ceil(s/64) + 1) bytes, each
 * part rounded up to 16, <= 159 KiB; tier 3 beyond), and ldpc_osd_postprocess_batch_device keeps its signature and its promises (in place, call
 * order).  The HOST form of this rule is out of scope: ldpc_osd_postprocess_batch on such a handle answers
 * LDPC_ERR_UNSUPPORTED and names the device entry. */
#include "ldpc_mi355x_osd_search.h"

/* ------------------------------------------------------------------------
 * BP-OTS decoder: LLR-domain tanh/atanh BP with oscillation-driven prior biasing.
 * Graphs whose messages fit one CU's LDS (every code of the reference's BP-OTS tests) take an LDS-resident
 * kernel; larger ones a node-parallel kernel with the messages in global memory, as long as s + 3n bytes of
 * decisions and 4s bytes of parities fit the LDS (n up to ~30,000 at rate 1/2) and no check has more than 32 or bit
 * more than 16 edges; anything beyond that a third kernel that keeps everything of a syndrome in global memory and
 * takes nodes of any degree -- like the reference's BPOTSDecoder, which takes any H.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_bpots_decoder ldpc_bpots_decoder;

/* Replaces `BPOTSDecoder(H, per, max_iters; T=9, C=2.0)` (src/decoders/bpots_decoder.jl:39-115);
 * H as the zero-based CSC pattern, like ldpc_bp_create.  device < 0: current device. */
ldpc_status ldpc_bpots_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr,
                              const int64_t *rowval, double per, int64_t max_iters, int64_t T, double C,
                              int32_t device, ldpc_bpots_decoder **out);
ldpc_status ldpc_bpots_destroy(ldpc_bpots_decoder *dec);
/* Which kernel this decoder's graph takes (numbered like ldpc_bp_options.kernel_variant): 2 = LDS-resident (S syndromes
 * per workgroup), 3 = node-parallel with the messages in a global slot (graphs beyond one CU's LDS), 5 = the same with
 * everything of a syndrome in the global slot and nodes of any degree (no size or degree limit); 0 for NULL. */
int32_t ldpc_bpots_kernel(const ldpc_bpots_decoder *dec);

/* Replaces `decode!(decoder::BPOTSDecoder, syndrome)` (:225-340, with its `reset!` :142-154) for a
 * batch, i.e. the generic `batchdecode!` (abstract_decoder.jl:31-48) over it.  HOST buffers.
 *   syndromes [batch][s] uint8 : a non-zero entry flips the check's sign (:195); entries other than
 *                                0/1 can never be matched (:273)
 *   errors    [batch][n] uint8 : `best_decisions` (:340), converged [batch] : a zero-mismatch
 *   estimate was found (:290), iters [batch] int32 (may be NULL): iterations executed (extension). */
ldpc_status ldpc_bpots_decode_batch(ldpc_bpots_decoder *dec, int64_t batch, const uint8_t *syndromes,
                                    uint8_t *errors, uint8_t *converged, int32_t *iters);
/* Same with DEVICE pointers, asynchronous on `stream`. */
ldpc_status ldpc_bpots_decode_batch_device(ldpc_bpots_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                           uint8_t *d_errors, uint8_t *d_converged, int32_t *d_iters,
                                           void *stream);

/* ------------------------------------------------------------------------
 * Bit-flip decoder: `BitFlipDecoder(H, per, max_iters)` (src/decoders/iterative_bitflip.jl:61-68), the reference's
 * fourth exported decoder.  Per syndrome, with err = 0 and votes = 0 once (reset!, :84-88), for iter = 1 .. max_iters:
 *   1. H * err mod 2 == syndrome: converged, stop (:122-127).  An entry other than 0/1 can never be equal.
 *   2. every check adds +1 (mismatched) or -1 (matched) to the vote of each of its bits (:131-143); the votes are NOT
 *      cleared between iterations.
 *   3. if the largest vote is >= 0, ONE bit among those that hold it is toggled (:145-149); otherwise the loop stops
 *      and reports converged = true although the syndrome is not matched (:150-152: what the code does).
 * Everything but the choice in step 3 -- `rand(max_idxs)` in the reference -- is integer arithmetic with one legal
 * outcome, so the output is the reference's for SOME realisation of its rand calls, and this header says which:
 *
 * The tie rule.  The candidates (bits whose vote equals the maximum) are ordered by ascending bit index, k of them.
 * LDPC_BF_TIE_FIRST takes candidate 0, LDPC_BF_TIE_LAST candidate k - 1.  LDPC_BF_TIE_RANDOM (default) takes candidate
 *     ((r >> 32) * k) >> 32,   r = mix(mix(seed + 0x9E3779B97F4A7C15 * (column0 + i + 1)) + iter)
 * in uint64 arithmetic, where mix is the SplitMix64 finaliser
 *     z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * i is the column's index in the call and iter the 1-based iteration.  No state is carried from call to call: column i
 * of a call with column0 = c is decoded exactly like column 0 of a call with column0 = c + i, whatever kernel, chunking
 * or stream is used.
 *
 * These entries were added WITHOUT a change of LDPC_MI355X_ABI_VERSION (they only add symbols): a caller detects them
 * by symbol lookup, like the bits entries.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_bitflip_decoder ldpc_bitflip_decoder;

enum { LDPC_BF_TIE_RANDOM = 0, LDPC_BF_TIE_FIRST = 1, LDPC_BF_TIE_LAST = 2 };

/* Optional; pass NULL to ldpc_bitflip_create for defaults (current device, LDPC_BF_TIE_RANDOM, seed 0, auto). */
typedef struct ldpc_bitflip_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t tie_break;       /* LDPC_BF_TIE_* */
    uint64_t seed;           /* of the RANDOM rule */
    int32_t kernel_variant;  /* 0 = auto; 1, 2, 3 force that tier of ldpc_bitflip_kernel (1, 2: LDPC_ERR_UNSUPPORTED when
                                the state of a syndrome does not fit it) */
    int32_t reserved[11];
} ldpc_bitflip_options;

/* H as the zero-based CSC pattern with the checks of ldpc_bp_create (ascending rows, in range).  EVERY stored entry is
 * an edge: the reference reads the stored values (`sparse_H[i, j]`, `sparse_H * err`), so a caller that holds stored
 * `false` entries drops them first (`dropzeros`; both Julia shims do).  `per` is stored, nothing computes with it (as
 * in the reference).  The vote accumulators are exact: 32-bit when max_iters * (largest bit degree) < 2^31, 64-bit
 * otherwise.  tie_break outside 0..2 / kernel_variant outside 0..3: LDPC_ERR_INVALID_ARGUMENT. */
ldpc_status ldpc_bitflip_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                                double per, int64_t max_iters, const ldpc_bitflip_options *options,
                                ldpc_bitflip_decoder **out);
ldpc_status ldpc_bitflip_destroy(ldpc_bitflip_decoder *dec);
/* Which tier this decoder's graph takes: 1 = on-chip (state in LDS), one wave per syndrome (n <= 2048, <= 40 KiB of
 * state); 2 = on-chip, one 16-wave workgroup per syndrome (<= 159 KiB of state: 9 n + s + n / 16 bytes); 3 = unlimited
 * (state in a global workspace; any H with nnz < 2^28); 4 = unlimited with 64-bit votes; 0 for NULL. */
int32_t ldpc_bitflip_kernel(const ldpc_bitflip_decoder *dec);

/* Replaces `batchdecode!(decoder::BitFlipDecoder, syndromes, errors, converged)` (:189-201) and, with batch = 1,
 * `decode!` (:116-157).  HOST buffers, laid out as for ldpc_bp_decode_batch.
 *   syndromes   [batch][s] uint8  in
 *   errors      [batch][n] uint8  out: err (:156)
 *   converged   [batch]    uint8  out: the reference's flag (1 for stop reasons 1 AND 2)
 *   iters       [batch]    int32  out, may be NULL: loop iterations entered (the one that stops counts; 0 for max_iters = 0)
 *   stop_reason [batch]    uint8  out, may be NULL: 0 = ran out of iterations, 1 = syndrome matched, 2 = no bit with a
 *                                 non-negative vote (with n = 0 there is no bit at all: reason 2 as well)
 *   column0 >= 0: the number the first column of this call carries in the tie rule above.
 * max_iters = 0: zeros, converged = 0.  batch = 0: LDPC_OK, nothing touched.  A NULL handle, a negative batch or
 * column0, a NULL pointer where ldpc_bp_decode_batch rejects one: LDPC_ERR_INVALID_ARGUMENT before any device work. */
ldpc_status ldpc_bitflip_decode_batch(ldpc_bitflip_decoder *dec, int64_t batch, int64_t column0, const uint8_t *syndromes,
                                      uint8_t *errors, uint8_t *converged, int32_t *iters, uint8_t *stop_reason);
/* Same with DEVICE pointers, asynchronous on `stream`; calls on one handle execute in call order: a call given another
 * stream than its predecessor waits (on the device) for that predecessor first. */
ldpc_status ldpc_bitflip_decode_batch_device(ldpc_bitflip_decoder *dec, int64_t batch, int64_t column0,
                                             const uint8_t *d_syndromes, uint8_t *d_errors, uint8_t *d_converged,
                                             int32_t *d_iters, uint8_t *d_stop_reason, void *stream);

/* ------------------------------------------------------------------------
 * Monte-Carlo trials on the device: what surrounds every decode in the reference's own use (test/test_bp_decoder.jl:19-30,
 * benchmark/benchmarks.jl:8-11) -- draw `errors = rand(n, B) .< per`, form `syndromes = H * errors .% 2`, decode, compare
 * `guesses[:, i] == errors[:, i]`, count.  A trials handle owns the Tanner graph of H and an optional second sparse
 * pattern L of nl x n "logical" rows, and offers the three steps around the decode with DEVICE pointers, so that the
 * batch never leaves the GPU and a run over many batches reads back the four counts.
 *
 * The sampling rule (a CPU model equals the device in every element).  mix is the SplitMix64 finaliser of the bit-flip
 * tie rule above; all arithmetic is uint64:
 *     k_i  = mix(seed + 0x9E3779B97F4A7C15 * (column0 + i + 1))        i = column index in the call
 *     r_ij = mix(k_i + j)                                              j = bit index
 *     t    = (uint64)(per * 18446744073709551616.0)                    for 0 <= per < 1 (a power-of-two scaling, truncated)
 *     error(i, j) = per >= 1 ? 1 : (r_ij < t)
 * per NaN, < 0 or > 1: LDPC_ERR_INVALID_ARGUMENT.  No state is carried between calls: column i of a call with
 * column0 = c equals column 0 of a call with column0 = c + i, whatever the tier, chunking or stream.
 *
 * Syndromes.  syndromes(i, r) = XOR over the stored entries (r, j) of H of errors(i, j) & 1.
 *
 * Score, per column i, with d = guesses(i, .) ^ errors(i, .) (low bits):
 *     flag bit 0: d != 0                 (the reference's `guess != err`)
 *     flag bit 1: H * d != 0             (the guess does not reproduce the error's syndrome)
 *     flag bit 2: L * d != 0 in some row (a logical failure; never set when nl = 0)
 * counts[0] += batch, counts[1..3] += the number of columns with each bit set.  Counts are ACCUMULATED, never zeroed by
 * the library: the caller zeroes them once, a run over many batches reads them back once.
 *
 * Layouts as everywhere in this header: errors / guesses [batch][n] bytes, syndromes [batch][s] bytes, flags [batch]
 * bytes.  H and L are zero-based CSC patterns with the checks of ldpc_bp_create (L has n columns); nl = 0 with NULL
 * lcolptr / lrowval is legal.  No pointer needs an alignment; score is fastest where d_guesses and d_errors agree in
 * address mod 16 (otherwise the guesses are read byte by byte: same result, 16 loads for one).  A call takes at most
 * 2^36 columns (more: LDPC_ERR_UNSUPPORTED).
 *
 * ldpc_trials_kernel: 1 = on-chip bit image (a column's bits, or those of d, live in LDS while its checks are walked:
 * n <= 1,302,497, i.e. 2 * ((n + 30) / 16 + 1) <= 159 KiB; columns of n <= 4096 bits take one wave each, four to a
 * workgroup, longer ones a workgroup each); 2 = unlimited (the walks read the bytes from global memory); 0 for NULL.
 * options->kernel_variant 0 = by size, 1 / 2 force a tier (1 where the image does not fit: LDPC_ERR_UNSUPPORTED).
 *
 * The *_device entries take DEVICE pointers and are asynchronous on `stream`; calls on one handle run in call order
 * whatever streams they are given.  ldpc_trials_sample and ldpc_trials_score take HOST buffers and are synchronous
 * (their waits are bounded by ldpc_set_wait_limit_ms); the host form's counts[4] is accumulated into as well.
 * d_syndromes / syndromes may be NULL in sample (errors only), d_flags / flags may be NULL in score; every other
 * pointer is required.  batch = 0: LDPC_OK, nothing touched.  A negative batch or column0, a per outside [0, 1], a NULL
 * required pointer, a NULL handle: LDPC_ERR_INVALID_ARGUMENT before any device work.  Without a device,
 * ldpc_trials_create returns LDPC_ERR_NO_DEVICE.
 *
 * Per-bit rates (biased noise, the columns of a detector error model: one rate per error mechanism).  A handle may hold
 * a table of n rates, set by ldpc_trials_set_rates; ldpc_trials_sample_rates[_device] then draws bit j at rates[j] by the
 * same stateless rule, with k_i, r_ij and mix exactly those above.  For rates[j], a double in [0, 1]:
 *     t_j         = (uint64)(rates[j] * 18446744073709551616.0)       for rates[j] < 1
 *     error(i, j) = rates[j] >= 1 ? 1 : (r_ij < t_j)
 * With rates[j] = per for all j, every element equals ldpc_trials_sample at that per, seed and column0 (per = 0 and
 * per = 1 included).  On the device the table is one uint64 threshold per bit; the largest double below 1 gives
 * t = 2^64 - 2^11, so the all-ones word never occurs for a rate below 1 and marks "always".
 * ldpc_trials_set_rates takes a HOST pointer and is synchronous: it validates, converts and uploads, ordered after every
 * earlier call on the handle (a sample still in flight keeps the table it was launched with; the wait for it is
 * bounded).  n must equal the handle's n; a rate that is NaN, < 0 or > 1: LDPC_ERR_INVALID_ARGUMENT, the message names
 * the first offending index, nothing is uploaded and the table set before stays in force.  rates = NULL clears the
 * table.  The two sample entries are ldpc_trials_sample[_device] without `per` in every other respect (d_syndromes may be
 * NULL, batch = 0 touches nothing, the 2^36 column limit, bounded waits, call order whatever the streams); without a
 * table they answer LDPC_ERR_INVALID_ARGUMENT before any device work.  ldpc_trials_syndromes* and ldpc_trials_score*
 * serve both kinds of sample.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_trials ldpc_trials;

/* Optional; pass NULL to ldpc_trials_create for defaults (current device, tier by size). */
typedef struct ldpc_trials_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_trials_kernel */
    int32_t reserved[14];
} ldpc_trials_options;

ldpc_status ldpc_trials_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                               int64_t nl, int64_t lnnz, const int64_t *lcolptr, const int64_t *lrowval,
                               const ldpc_trials_options *options, ldpc_trials **out);
ldpc_status ldpc_trials_destroy(ldpc_trials *t);
int32_t ldpc_trials_kernel(const ldpc_trials *t);
/* errors and (unless NULL) their syndromes in one pass */
ldpc_status ldpc_trials_sample_device(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed,
                                      uint8_t *d_errors, uint8_t *d_syndromes, void *stream);
/* the syndromes of given errors */
ldpc_status ldpc_trials_syndromes_device(ldpc_trials *t, int64_t batch, const uint8_t *d_errors,
                                         uint8_t *d_syndromes, void *stream);
ldpc_status ldpc_trials_score_device(ldpc_trials *t, int64_t batch, const uint8_t *d_guesses, const uint8_t *d_errors,
                                     uint8_t *d_flags, int64_t *d_counts, void *stream);
ldpc_status ldpc_trials_sample(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed,
                               uint8_t *errors, uint8_t *syndromes);
ldpc_status ldpc_trials_score(ldpc_trials *t, int64_t batch, const uint8_t *guesses, const uint8_t *errors,
                              uint8_t *flags, int64_t counts[4]);
/* per-bit rates: rates [n] doubles on the HOST, NULL clears the table */
ldpc_status ldpc_trials_set_rates(ldpc_trials *t, int64_t n, const double *rates);
ldpc_status ldpc_trials_sample_rates_device(ldpc_trials *t, int64_t batch, int64_t column0, uint64_t seed,
                                            uint8_t *d_errors, uint8_t *d_syndromes, void *stream);
ldpc_status ldpc_trials_sample_rates(ldpc_trials *t, int64_t batch, int64_t column0, uint64_t seed,
                                     uint8_t *errors, uint8_t *syndromes);

/* ------------------------------------------------------------------------
 * Monte-Carlo trials of a CSS code on the device: two check matrices Hx (rows_x x n) and Hz (rows_z x n) over the same n
 * qubits, Pauli errors (depolarizing or biased: the X part and the Z part of a qubit's error are correlated), two
 * syndromes for two decoders, and a joint score that counts logical X and logical Z failures.  A CSS trials handle owns
 * the Tanner graphs of Hx, Hz and of two optional patterns of logical rows Lx (nlx x n) and Lz (nlz x n).  The library
 * does not require Hx * Hz' = 0.
 *
 * The sampling rule (a CPU model equals the device in every element), with mix, k_i and r_ij of the trials section:
 *     k_i  = mix(seed + 0x9E3779B97F4A7C15 * (column0 + i + 1))        i = column index in the call
 *     r_ij = mix(k_i + j)                                              j = qubit
 *     tx, ty, tz = (uint64)(px * 2^64), (uint64)(py * 2^64), (uint64)(pz * 2^64)      each rate in [0, 1), truncated
 *     a = tx, b = tx + ty, c = tx + ty + tz                            uint64
 *     Pauli(i, j) = X if r < a, Y if a <= r < b, Z if b <= r < c, else I
 *     ex(i, j) = X or Y = (r < b)          ez(i, j) = Y or Z = (a <= r < c)
 * One mix per qubit feeds both arrays.  A rate that is NaN, negative or >= 1, or an overflow of either sum:
 * LDPC_ERR_INVALID_ARGUMENT.  No state is carried between calls: column i of a call with column0 = c equals column 0 of
 * a call with column0 = c + i, whatever the tier, batch or stream.  With py = pz = 0, ex equals the errors of
 * ldpc_trials_sample at per = px and the same seed, and ez is zero.
 *
 * Syndromes.  sz(i, r) = XOR over the stored entries (r, j) of Hz of ex(i, j) & 1 (the Z checks see the X part);
 *             sx(i, r) = XOR over the stored entries (r, j) of Hx of ez(i, j) & 1.
 *
 * Score, per column i, with dx = gx(i, .) ^ ex(i, .) and dz = gz(i, .) ^ ez(i, .) (low bits):
 *     flag bit 0: dx != 0 or dz != 0
 *     flag bit 1: Hz * dx != 0 or Hx * dz != 0
 *     flag bit 2: Lz * dx != 0 in some row (a logical X failure; never set when nlz = 0)
 *     flag bit 3: Lx * dz != 0 in some row (a logical Z failure; never set when nlx = 0)
 * counts[0] += batch, counts[1] += columns with bit 0, counts[2] += columns with bit 1, counts[3] += columns with bit 2
 * or bit 3, counts[4] += columns with bit 2, counts[5] += columns with bit 3.  Counts are ACCUMULATED, never zeroed by
 * the library.
 *
 * Layouts: ex / ez / gx / gz [batch][n] bytes, sx [batch][rows_x] bytes, sz [batch][rows_z] bytes, flags [batch] bytes.
 * Every pattern is a zero-based CSC pattern of n columns with the checks of ldpc_trials_create; lx / lz may be NULL or
 * have rows = 0 (then colptr / rowval are not read).  No pointer needs an alignment.  The 16-byte pieces of a column
 * are laid on its address in ex; every other array (ez; in score gx and gz) is fastest where it agrees with ex in
 * address mod 16 and is otherwise accessed byte by byte: same result, 16 accesses for one.  A call takes at most 2^36
 * columns (more: LDPC_ERR_UNSUPPORTED).
 *
 * ldpc_css_trials_kernel: 1 = on-chip bit images (a column's two images live in LDS while the checks are walked:
 * n <= 651,233, i.e. 2 * 2 * ((n + 30) / 16 + 1) <= 159 KiB with an image rounded up to 16 bytes; columns of n <= 4096
 * take one wave each, four to a workgroup, longer ones a workgroup each); 2 = unlimited (the walks read the bytes from
 * global memory); 0 for NULL.  options->kernel_variant 0 = by size, 1 / 2 force a tier (1 where the images do not fit:
 * LDPC_ERR_UNSUPPORTED).
 *
 * The *_device entries take DEVICE pointers and are asynchronous on `stream`; calls on one handle run in call order
 * whatever streams they are given.  ldpc_css_trials_sample and ldpc_css_trials_score take HOST buffers and are
 * synchronous (their waits are bounded by ldpc_set_wait_limit_ms); the host form's counts[6] is accumulated into as
 * well.  In sample, d_sx / sx and d_sz / sz may both be NULL (errors only; one of them alone:
 * LDPC_ERR_INVALID_ARGUMENT); d_flags / flags may be NULL in score; every other pointer is required.  batch = 0: LDPC_OK, nothing touched.  A negative batch or column0, a bad
 * rate, a NULL required pointer, a NULL handle: LDPC_ERR_INVALID_ARGUMENT before any device work.  Without a device,
 * ldpc_css_trials_create returns LDPC_ERR_NO_DEVICE.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_css_trials ldpc_css_trials;

/* A zero-based CSC pattern of `rows` rows (its column count is the n of the call). */
typedef struct ldpc_css_pattern {
    int64_t rows, nnz;
    const int64_t *colptr;   /* [n + 1] */
    const int64_t *rowval;   /* [nnz] */
} ldpc_css_pattern;

/* Optional; pass NULL to ldpc_css_trials_create for defaults (current device, tier by size). */
typedef struct ldpc_css_trials_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_css_trials_kernel */
    int32_t reserved[14];
} ldpc_css_trials_options;

ldpc_status ldpc_css_trials_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz,
                                   const ldpc_css_pattern *lx, const ldpc_css_pattern *lz,
                                   const ldpc_css_trials_options *options, ldpc_css_trials **out);
ldpc_status ldpc_css_trials_destroy(ldpc_css_trials *t);
int32_t ldpc_css_trials_kernel(const ldpc_css_trials *t);
/* Pauli errors and (unless NULL) their two syndromes in one pass */
ldpc_status ldpc_css_trials_sample_device(ldpc_css_trials *t, int64_t batch, int64_t column0, double px, double py,
                                          double pz, uint64_t seed, uint8_t *d_ex, uint8_t *d_ez, uint8_t *d_sx,
                                          uint8_t *d_sz, void *stream);
/* the two syndromes of given errors */
ldpc_status ldpc_css_trials_syndromes_device(ldpc_css_trials *t, int64_t batch, const uint8_t *d_ex,
                                             const uint8_t *d_ez, uint8_t *d_sx, uint8_t *d_sz, void *stream);
ldpc_status ldpc_css_trials_score_device(ldpc_css_trials *t, int64_t batch, const uint8_t *d_gx, const uint8_t *d_gz,
                                         const uint8_t *d_ex, const uint8_t *d_ez, uint8_t *d_flags, int64_t *d_counts,
                                         void *stream);
ldpc_status ldpc_css_trials_sample(ldpc_css_trials *t, int64_t batch, int64_t column0, double px, double py, double pz,
                                   uint64_t seed, uint8_t *ex, uint8_t *ez, uint8_t *sx, uint8_t *sz);
ldpc_status ldpc_css_trials_score(ldpc_css_trials *t, int64_t batch, const uint8_t *gx, const uint8_t *gz,
                                  const uint8_t *ex, const uint8_t *ez, uint8_t *flags, int64_t counts[6]);

/* ------------------------------------------------------------------------
 * Normalised min-sum decoder with one channel LLR per bit.  Not a decoder of the reference: it is what the uniform
 * `per` of every other create cannot express (biased noise, the two sides of a CSS code, soft input, detector-error-model
 * columns), and it has no division and no transcendental function, so THE RULE below has one legal outcome in IEEE
 * binary32 and a numpy model equals the device in every bit, LLRs included.
 *
 * Inputs.  H as a zero-based CSC pattern with the checks of ldpc_bp_create.  channel_llr[n] binary32 =
 * log(P(bit = 0) / P(bit = 1)), each finite; the library calls no log or exp, the caller computes the array.
 * alpha binary32 in (0, 1] (default 0.75), clip binary32 finite and > 0 (default 1.0e6f), max_iters >= 0.  A syndrome
 * entry that is not 0 counts as 1.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * State per syndrome: L[j], initially channel_llr[j]; the check-to-bit messages c[i][j], initially +0.
 * For t = 1 .. max_iters:
 *   1. Check sweep.  For check i with its bits j_0 < j_1 < ... (ascending):
 *        b_k = min(max(L[j_k] - c[i][j_k], -clip), clip);   neg_k = (b_k < 0);   mag_k = |b_k|
 *        m1 = m2 = clip, a = none; for k ascending: if mag_k < m1 { m2 = m1; m1 = mag_k; a = k } else if mag_k < m2 { m2 = mag_k }
 *        par = syndrome_i XOR neg_0 XOR neg_1 XOR ...
 *        new c[i][j_k]: the value alpha * (k == a ? m2 : m1), with its sign bit set iff par XOR neg_k (a zero product
 *        with the sign set is -0).  All b_k are formed from the old messages before any is replaced.  A check with no
 *        bits sends nothing.
 *   2. Bit sweep.  L[j] = channel_llr[j] + c[i_0][j] + c[i_1][j] + ..., added one after another from the left in ascending
 *      check order; err[j] = (L[j] <= 0).
 *   3. Stop test.  If H * err == syndrome (an empty check is matched only by a 0 entry): converged = 1, iters = t, stop;
 *      L and err stay as they are.
 * Not stopped after max_iters: converged = 0, iters = max_iters.  With finite inputs no NaN or infinity can arise.
 * The form "L - c" (total minus own message) is part of the rule: it lets a kernel keep L and, per check, only
 * (alpha m1, alpha m2, a, the sign bits).
 *
 * THE LAYERED RULE (options->schedule = 1; the rule above is the flooding schedule, 0).  A check reads the L that the
 * checks before it have just updated, so there is no bit sweep.  Same arithmetic: binary32, every operation rounded
 * once, no fused multiply-add, subnormals kept.
 *   Layers.  Go through the checks in ascending index.  A check with no bits belongs to no layer.  Every other check goes
 *   into the lowest-numbered layer that so far holds no check sharing a bit with it (first fit).  K = the number of
 *   layers; inside a layer the checks are in ascending order.  The assignment is part of the rule: the order of the
 *   updates changes the result.
 *   State per syndrome: L[j], initially channel_llr[j]; c[i][j], initially +0.  For t = 1 .. max_iters:
 *   1. Go through the layers 0 .. K - 1 in order.  For every check i of the layer with its bits j_0 < j_1 < ...:
 *        b_k = min(max(L[j_k] - c[i][j_k], -clip), clip);  neg_k, mag_k, m1, m2, a and par exactly as in step 1 above;
 *        new c[i][j_k]: the value alpha * (k == a ? m2 : m1), with its sign bit set iff par XOR neg_k;
 *        then L[j_k] = b_k + c[i][j_k], with the clamped b_k and the new message.
 *      All b_k of a check are formed before any of its L or c is replaced.  The checks of one layer share no bit, so
 *      their order is free.
 *   2. After the last layer err[j] = (L[j] <= 0).  If H * err == syndrome (an empty check is matched only by a 0 entry):
 *      converged = 1, iters = t, stop; L and err stay as they are.
 * Not stopped after max_iters: converged = 0, iters = max_iters.  max_iters = 0 as below.  A bit of degree 0 keeps its
 * prior.  ldpc_minsum_layers: K of a layered handle; 0 for a flooding handle and for NULL.
 *
 * Outputs.  errors [batch][n] uint8; converged [batch] uint8; llr [batch][n] DOUBLE (may be NULL): L widened exactly,
 * so it feeds ldpc_osd_postprocess_batch[_device] as it is; iters [batch] int32 (may be NULL).  max_iters = 0: zeros,
 * converged = 0, llr = 0, iters = 0.  batch = 0: LDPC_OK, nothing touched.
 *
 * ldpc_minsum_kernel: 1 = on-chip (L and the check records of the S <= 64 syndromes a workgroup holds live in LDS for
 * the whole decode; needs (4 (n + record words) + s) bytes <= 159 KiB for one syndrome, a record being 4 words for a
 * check of degree <= 32, 5 up to 64, one word per edge beyond); 2 = unlimited (tiles of 64 syndromes in a workspace the
 * handle owns, sized by the resident workgroups; any H with nnz < 2^28); 0 for NULL.  options->kernel_variant 0 = by
 * size, 1 / 2 force a tier (1 where the state does not fit: LDPC_ERR_UNSUPPORTED).
 *
 * ldpc_minsum_tile_syndromes: the S of the handle -- on-chip the largest power of two <= 64 whose state fits 79 KiB (two
 * workgroups a CU), else the largest that fits 159 KiB; 64 in the unlimited tier; 0 for NULL.  ldpc_minsum_last_grid: the
 * workgroups of the handle's most recent kernel launch (each takes tile after tile of S syndromes in the same LDS block
 * or workspace slot, so a value below ceil(batch / S) means slots were reused); 0 before any launch and for NULL.  Both
 * only report what ran; neither has a reference counterpart.
 *
 * ldpc_minsum_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for a NULL or non-finite channel_llr,
 * alpha outside (0, 1], clip not in (0, inf), a kernel_variant outside 0..2, a schedule outside 0..1 and a pattern
 * ldpc_bp_create rejects;
 * without a device LDPC_ERR_NO_DEVICE.  The decode entries reject a NULL handle, a negative batch and a NULL required
 * pointer the same way.  ldpc_minsum_decode_batch takes HOST buffers and is synchronous (its wait is bounded by
 * ldpc_set_wait_limit_ms); ldpc_minsum_decode_batch_device takes DEVICE pointers and is asynchronous on `stream`; calls
 * on one handle run in call order whatever streams they are given.
 *
 * PER-SYNDROME PRIORS (ldpc_minsum_decode_batch_priors*, ldpc_minsum_decode_batch_given*).  Column i of the call is
 * decoded exactly by THE RULE (or THE LAYERED RULE, by the handle's schedule) with every occurrence of channel_llr[j] --
 * the initial L[j] and the left-most addend of the bit sweep -- replaced by priors[i][j].  Same arithmetic: binary32,
 * every operation rounded once, no fused multiply-add, subnormals kept; a numpy model equals the device in every bit,
 * LLRs included.  The handle's channel_llr plays no part in these entries.  Two sources of priors[i][j]:
 *   Floats.  priors [batch][n] binary32, laid out like every other batch array; no alignment is asked for.
 *   Given bits.  The handle holds two tables llr_if0[n], llr_if1[n], binary32 and finite, set by
 *     ldpc_minsum_set_conditional_priors (host arrays; may be called again: it waits for the earlier calls on the handle
 *     and takes effect for the calls after it); the call brings given [batch][n] uint8 and
 *     priors[i][j] = (given[i][j] & 1) ? llr_if1[j] : llr_if0[j]  -- the low bit, as the trial scores read a guess.  This
 *     is the second stage of a correlated decode of a CSS code (given = the other side's guess) at one byte per bit.
 * A column that holds a non-finite prior (only the floats form can) is not decoded: errors zeros, converged 0, iters 0,
 * llr 0 -- what max_iters = 0 writes; no other column is affected.  +-0 and subnormal priors are ordinary values.
 * max_iters = 0 and batch = 0 as above.
 * The flooding schedule keeps a tile's priors beside its state, 4 n more bytes per syndrome (the layered one reads them
 * only when a tile starts and keeps nothing), so these entries have a plan of their own, chosen at create by the same
 * policy: ldpc_minsum_priors_kernel and ldpc_minsum_priors_tile_syndromes report its tier and S (0 for NULL); for a
 * layered handle they equal ldpc_minsum_kernel / ldpc_minsum_tile_syndromes.  On a handle forced on-chip
 * (kernel_variant 1) whose state with the priors does not fit 159 KiB for one syndrome, create and the plain entries
 * succeed, both getters answer 0 and these entries answer LDPC_ERR_UNSUPPORTED.  ldpc_minsum_last_grid reports the most
 * recent launch of any entry.
 * Before any device work: LDPC_ERR_INVALID_ARGUMENT for a NULL handle, a negative batch, a NULL required pointer
 * (d_priors / d_given included), a NULL or non-finite table entry, and for a given entry on a handle without tables.
 * The forms without _device take HOST buffers and are synchronous (bounded waits); calls on one handle run in call
 * order whatever streams they are given, these entries included.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_minsum_decoder ldpc_minsum_decoder;

/* Optional; pass NULL to ldpc_minsum_create for defaults.  A zeroed struct means defaults too, except `device` (0 is
 * device 0; -1 = the current one): alpha = 0 / clip = 0 select 0.75 / 1.0e6f. */
typedef struct ldpc_minsum_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the bit-to-check values, finite, > 0; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_minsum_kernel */
    int32_t schedule;        /* 0 = flooding, 1 = layered (THE LAYERED RULE above); took reserved[0], the struct stays 64 bytes */
    int32_t reserved[11];
} ldpc_minsum_options;

ldpc_status ldpc_minsum_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                               const float *channel_llr, int64_t max_iters, const ldpc_minsum_options *options,
                               ldpc_minsum_decoder **out);
ldpc_status ldpc_minsum_destroy(ldpc_minsum_decoder *dec);
int32_t ldpc_minsum_kernel(const ldpc_minsum_decoder *dec);
int32_t ldpc_minsum_tile_syndromes(const ldpc_minsum_decoder *dec);
int32_t ldpc_minsum_last_grid(const ldpc_minsum_decoder *dec);
int32_t ldpc_minsum_layers(const ldpc_minsum_decoder *dec);
ldpc_status ldpc_minsum_decode_batch(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *syndromes, uint8_t *errors,
                                     uint8_t *converged, double *llr, int32_t *iters);
ldpc_status ldpc_minsum_decode_batch_device(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                            uint8_t *d_errors, uint8_t *d_converged, double *d_llr, int32_t *d_iters,
                                            void *stream);
/* per-syndrome priors (PER-SYNDROME PRIORS above) */
int32_t ldpc_minsum_priors_kernel(const ldpc_minsum_decoder *dec);
int32_t ldpc_minsum_priors_tile_syndromes(const ldpc_minsum_decoder *dec);
ldpc_status ldpc_minsum_decode_batch_priors(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *syndromes,
                                            const float *priors, uint8_t *errors, uint8_t *converged, double *llr,
                                            int32_t *iters);
ldpc_status ldpc_minsum_decode_batch_priors_device(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                                   const float *d_priors, uint8_t *d_errors, uint8_t *d_converged,
                                                   double *d_llr, int32_t *d_iters, void *stream);
ldpc_status ldpc_minsum_set_conditional_priors(ldpc_minsum_decoder *dec, const float *llr_if0, const float *llr_if1);
ldpc_status ldpc_minsum_decode_batch_given(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *syndromes,
                                           const uint8_t *given, uint8_t *errors, uint8_t *converged, double *llr,
                                           int32_t *iters);
ldpc_status ldpc_minsum_decode_batch_given_device(ldpc_minsum_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                                  const uint8_t *d_given, uint8_t *d_errors, uint8_t *d_converged,
                                                  double *d_llr, int32_t *d_iters, void *stream);

/* ------------------------------------------------------------------------
 * Joint X/Z (Pauli) min-sum decoder of a CSS code: ONE decoder over both check matrices.  Every other decoder here is
 * binary and sees one side of the code; under depolarizing noise a Y error flips both sides, and two binary decoders
 * throw that correlation away.  Here each qubit carries three beliefs (X, Y, Z against I) and both kinds of check send
 * the scalar min-sum messages of ldpc_minsum_* (quaternary belief propagation with scalar messages, in its min-sum
 * form).  Not a decoder of the reference.  Compare, add and one multiply in binary32, no division and no transcendental
 * function, so THE RULE below has one legal outcome in IEEE binary32 and a numpy model equals the device in every bit,
 * LLRs included.  Flooding schedule only.
 *
 * Inputs.  hx with rx rows and hz with rz rows, both zero-based CSC patterns over the same n qubits (ldpc_css_pattern, as
 * ldpc_css_trials_create takes them), rx >= 1 and rz >= 1.  The checks are numbered Hx rows first (0 .. rx - 1), then Hz
 * rows (rx .. rx + rz - 1).  prior_x[n], prior_y[n], prior_z[n] binary32, each finite: log(P(I) / P(W)) of the qubit for
 * W = X, Y, Z; the library calls no log, the caller computes the arrays.  alpha, clip, max_iters: as ldpc_minsum_create
 * takes them.  Syndromes sx [batch][rx] (= Hx ez: an Hx row sees the Z parts) and sz [batch][rz] (= Hz ex: an Hz row sees
 * the X parts); an entry that is not 0 counts as 1.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * min(x, y) below means  x < y ? x : y  with the operands in the order given.
 * State per syndrome: TX[j], TZ[j], initially +0; the check-to-qubit messages c[i][j], initially +0.
 * Derived, wherever used:  GX[j] = prior_x[j] + TX[j];  GZ[j] = prior_z[j] + TZ[j];  GY[j] = (prior_y[j] + TX[j]) + TZ[j].
 * For t = 1 .. max_iters:
 *   1. Check sweep.  For check i with its qubits j_0 < j_1 < ... (ascending), with G of j_k:
 *        an Hx row (sees Z parts):  u_k = min(GY, GZ);  w_k = GX < 0 ? GX : +0
 *        an Hz row (sees X parts):  u_k = min(GY, GX);  w_k = GZ < 0 ? GZ : +0
 *        b_k = min(max((u_k - c[i][j_k]) - w_k, -clip), clip);   neg_k = (b_k < 0);   mag_k = |b_k|
 *        m1, m2, a, par and the new c[i][j_k] exactly as in step 1 of THE RULE of ldpc_minsum_*: par starts from the
 *        check's own syndrome entry (sx_i or sz_{i - rx}); the new message is alpha * (k == a ? m2 : m1) with its sign
 *        bit set iff par XOR neg_k.  All b_k are formed from the old state before any message is replaced.  A check with
 *        no qubits sends nothing.
 *   2. Bit sweep.  TX[j] = ((+0 + c[i_0][j]) + c[i_1][j]) + ... over the Hz checks of j in ascending order; TZ[j] the same
 *      sum over the Hx checks of j.  Decision:  best = X, g = GX;  if GZ < g { best = Z, g = GZ };  if GY < g { best = Y,
 *      g = GY };  E = (g <= 0) ? best : I;  ex[j] = (E is X or Y);  ez[j] = (E is Z or Y).
 *   3. Stop test.  If Hz ex == sz and Hx ez == sx (an empty check is matched only by a 0 entry): converged = 1, iters = t,
 *      stop; TX, TZ, ex and ez stay as they are.
 * Not stopped after max_iters: converged = 0, iters = max_iters.  With finite inputs no NaN or infinity can arise.
 * The form "total minus own message" (u_k contains c[i][j_k]; it is subtracted) is part of the rule: it lets a kernel
 * keep TX, TZ and, per check, only (alpha m1, alpha m2, a, the sign bits).
 *
 * Outputs.  gx [batch][n] uint8 = ex and gz [batch][n] uint8 = ez (what ldpc_css_trials_score_device reads as guesses);
 * converged [batch] uint8; iters [batch] int32 (may be NULL); llr [batch][3][n] DOUBLE (may be NULL): the planes GX, GY,
 * GZ of the final state widened exactly.  max_iters = 0: zeros everywhere, llr included.  batch = 0: LDPC_OK, nothing
 * touched.
 *
 * ldpc_pauli_minsum_kernel: 1 = on-chip (TX, TZ and the check records of the S <= 64 syndromes a workgroup holds live in
 * LDS for the whole decode; needs (4 (2 n + record words) + rx + rz) bytes <= 159 KiB for one syndrome, records as in
 * ldpc_minsum_kernel over the checks of both sides); 2 = unlimited (tiles of 64 syndromes in a workspace the handle owns);
 * 0 for NULL.  options->kernel_variant 0 = by size, 1 / 2 force a tier (1 where the state does not fit:
 * LDPC_ERR_UNSUPPORTED).  ldpc_pauli_minsum_tile_syndromes and ldpc_pauli_minsum_last_grid: as
 * ldpc_minsum_tile_syndromes and ldpc_minsum_last_grid, by the same policy over that state.
 *
 * ldpc_pauli_minsum_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for a NULL or non-finite prior,
 * alpha outside (0, 1], clip not in (0, inf), a kernel_variant outside 0..2, a NULL pattern or one ldpc_bp_create rejects
 * on either side, and rx < 1 or rz < 1; without a device LDPC_ERR_NO_DEVICE.  The library does not check that Hx and Hz
 * commute.  The decode entries reject a NULL handle, a negative batch and a NULL required pointer the same way.
 * ldpc_pauli_minsum_decode_batch takes HOST buffers and is synchronous (its wait is bounded by ldpc_set_wait_limit_ms);
 * ldpc_pauli_minsum_decode_batch_device takes DEVICE pointers and is asynchronous on `stream`; calls on one handle run in
 * call order whatever streams they are given.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_pauli_minsum_decoder ldpc_pauli_minsum_decoder;

/* Optional; pass NULL to ldpc_pauli_minsum_create for defaults.  A zeroed struct means defaults too, except `device` (0
 * is device 0; -1 = the current one): alpha = 0 / clip = 0 select 0.75 / 1.0e6f. */
typedef struct ldpc_pauli_minsum_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the qubit-to-check values, finite, > 0; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_pauli_minsum_kernel */
    int32_t reserved[12];
} ldpc_pauli_minsum_options;

ldpc_status ldpc_pauli_minsum_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz,
                                     const float *prior_x, const float *prior_y, const float *prior_z, int64_t max_iters,
                                     const ldpc_pauli_minsum_options *options, ldpc_pauli_minsum_decoder **out);
ldpc_status ldpc_pauli_minsum_destroy(ldpc_pauli_minsum_decoder *dec);
int32_t ldpc_pauli_minsum_kernel(const ldpc_pauli_minsum_decoder *dec);
int32_t ldpc_pauli_minsum_tile_syndromes(const ldpc_pauli_minsum_decoder *dec);
int32_t ldpc_pauli_minsum_last_grid(const ldpc_pauli_minsum_decoder *dec);
ldpc_status ldpc_pauli_minsum_decode_batch(ldpc_pauli_minsum_decoder *dec, int64_t batch, const uint8_t *sx, const uint8_t *sz,
                                           uint8_t *gx, uint8_t *gz, uint8_t *converged, double *llr, int32_t *iters);
ldpc_status ldpc_pauli_minsum_decode_batch_device(ldpc_pauli_minsum_decoder *dec, int64_t batch, const uint8_t *d_sx,
                                                  const uint8_t *d_sz, uint8_t *d_gx, uint8_t *d_gz, uint8_t *d_converged,
                                                  double *d_llr, int32_t *d_iters, void *stream);

/* ------------------------------------------------------------------------
 * Relay min-sum decoder: normalised min-sum with a per-bit MEMORY, run as a chain of LEGS, returning the solution of
 * lowest prior weight among the first `stop_after` it finds.  For the degenerate, short-cycle graphs of quantum LDPC
 * codes, where plain min-sum stalls.  Like ldpc_minsum_* it has no division and no transcendental function, so THE
 * RULE below has one legal outcome in IEEE binary32 and a numpy model equals the device in every bit.
 *
 * Inputs.  H, channel_llr[n], alpha, clip: as ldpc_minsum_create takes them.  legs >= 1; gammas[legs][n] binary32, the
 * memory strengths, each finite with -1 < gamma < 1 (negative values are meaningful); leg_iters[legs] int32, each >= 0,
 * their sum at most INT32_MAX; stop_after >= 1 (default 1).  The library draws no random number: the caller supplies
 * gammas.  A syndrome entry that is not 0 counts as 1.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * Derived once per handle:
 *   g0[r][j] = (1.0f - gammas[r][j]) * channel_llr[j]                  (one subtraction, one multiplication)
 *   q[j]     = (int64) rint(clamp((double) channel_llr[j], -2^24, 2^24) * 2^16)      (the product is exact in double)
 * n > 2^22 answers LDPC_ERR_UNSUPPORTED, so a weight (a sum of q[j]) always fits int64.
 * State per syndrome: the posterior M[j], initially channel_llr[j]; X[j]; the check-to-bit messages c[i][j];
 * found = 0, iters = 0; best, an error pattern, and its weight best_w.
 * For leg r = 0 .. legs - 1 (a leg with leg_iters[r] = 0 is skipped):
 *   Leg start.  Every c <- +0;  X[j] = g0[r][j] + gammas[r][j] * M[j]   (multiply, then add).
 *   For t = 1 .. leg_iters[r]:
 *     1. Check sweep: step 1 of the min-sum rule above with X in the place of L -- b_k = min(max(X[j_k] - c[i][j_k],
 *        -clip), clip), the same ascending scan for m1, m2, a, the same par and the same signed alpha * (k == a ? m2 : m1),
 *        -0 included; all b_k of a check are formed from the old messages.
 *     2. Bit sweep, for every j:  Lambda = g0[r][j] + gammas[r][j] * M[j] with the OLD M;
 *        M[j] = Lambda + c[i_0][j] + c[i_1][j] + ... from the left, checks ascending;  then with the NEW M:
 *        Lambda' = g0[r][j] + gammas[r][j] * M[j],  X[j] = Lambda' + c[i_0][j] + c[i_1][j] + ... in the same order.
 *        err[j] = (M[j] <= 0);  iters += 1.
 *     3. Test.  If H * err == syndrome (an empty check is matched only by a 0 entry):  w = sum over j of err[j] * q[j]
 *        in int64 (exact, so any summation order is legal);  if found == 0 or w < best_w: best = err, best_w = w (a tie
 *        keeps the earlier solution);  found += 1;  if found == stop_after the syndrome stops, otherwise the leg ends
 *        and the next leg starts from this M.
 *   A leg that uses up leg_iters[r] without a solution ends, and the next starts from its M.
 * After the last leg the syndrome stops.
 *
 * Outputs.  errors [batch][n] uint8 = best if found > 0, else (M <= 0) as it stands; converged [batch] uint8 =
 * (found > 0); iters [batch] int32 (may be NULL): the total over all legs; solutions [batch] int32 (may be NULL) = found;
 * llr [batch][n] DOUBLE (may be NULL): M as it stands when the syndrome stops, widened exactly -- with found > 1 that is
 * the M of the LAST solution (or of the last iteration), not necessarily the M of `best`.  Every leg of 0 iterations:
 * zeros, converged = 0, llr = 0, iters = 0, solutions = 0, as max_iters = 0 of min-sum.  batch = 0: LDPC_OK, nothing
 * touched.
 *
 * Consequence.  With legs = 1, gammas all 0, stop_after = 1 and no channel_llr equal to -0, every output equals
 * ldpc_minsum_* with max_iters = leg_iters[0] in every bit:  (1 - 0) * p = p  and  p + (+-0) = p.
 *
 * ldpc_relay_kernel: 1 = on-chip (X, M, the check records, best and the syndromes of the S <= 64 syndromes a workgroup
 * holds live in LDS for the whole decode; needs (4 (2 n + record words + ceil(n / 32)) + s) bytes <= 159 KiB for one
 * syndrome, records as in ldpc_minsum_kernel); 2 = unlimited (tiles of 64 syndromes in a workspace the handle owns,
 * sized by the resident workgroups; any H with nnz < 2^28); 0 for NULL.  options->kernel_variant 0 = by size, 1 / 2 force
 * a tier (1 where the state does not fit: LDPC_ERR_UNSUPPORTED).
 *
 * ldpc_relay_tile_syndromes, ldpc_relay_last_grid: as ldpc_minsum_tile_syndromes and ldpc_minsum_last_grid -- the S of
 * the handle, and the workgroups of its most recent kernel launch (0 before any launch); 0 for NULL.
 *
 * ldpc_relay_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for a NULL channel_llr, gammas or
 * leg_iters, a non-finite channel_llr, a gamma that is not finite or outside (-1, 1), legs < 1, a negative leg_iters
 * entry, a leg_iters sum beyond INT32_MAX, stop_after < 0 (0 = default 1), alpha or clip outside their min-sum ranges,
 * a kernel_variant outside 0..2 and a pattern ldpc_bp_create rejects; without a device LDPC_ERR_NO_DEVICE.  The decode
 * entries behave as those of ldpc_minsum_*: ldpc_relay_decode_batch takes HOST buffers and is synchronous (its wait is
 * bounded by ldpc_set_wait_limit_ms); ldpc_relay_decode_batch_device takes DEVICE pointers and is asynchronous on
 * `stream`; calls on one handle run in call order whatever streams they are given.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_relay_decoder ldpc_relay_decoder;

/* Optional; pass NULL to ldpc_relay_create for defaults.  A zeroed struct means defaults too, except `device` (0 is
 * device 0; -1 = the current one): alpha = 0 / clip = 0 / stop_after = 0 select 0.75 / 1.0e6f / 1. */
typedef struct ldpc_relay_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the bit-to-check values, finite, > 0; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_relay_kernel */
    int32_t stop_after;      /* solutions to collect before a syndrome stops; 0 = default 1 */
    int32_t reserved[11];
} ldpc_relay_options;

ldpc_status ldpc_relay_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                              const float *channel_llr, int64_t legs, const float *gammas, const int32_t *leg_iters,
                              const ldpc_relay_options *options, ldpc_relay_decoder **out);
ldpc_status ldpc_relay_destroy(ldpc_relay_decoder *dec);
int32_t ldpc_relay_kernel(const ldpc_relay_decoder *dec);
int32_t ldpc_relay_tile_syndromes(const ldpc_relay_decoder *dec);
int32_t ldpc_relay_last_grid(const ldpc_relay_decoder *dec);
ldpc_status ldpc_relay_decode_batch(ldpc_relay_decoder *dec, int64_t batch, const uint8_t *syndromes, uint8_t *errors,
                                    uint8_t *converged, double *llr, int32_t *iters, int32_t *solutions);
ldpc_status ldpc_relay_decode_batch_device(ldpc_relay_decoder *dec, int64_t batch, const uint8_t *d_syndromes,
                                           uint8_t *d_errors, uint8_t *d_converged, double *d_llr, int32_t *d_iters,
                                           int32_t *d_solutions, void *stream);

/* ------------------------------------------------------------------------
 * Guided-decimation min-sum decoder (belief propagation with guided decimation, BPGD): normalised min-sum in ROUNDS of
 * round_iters iterations; a round that ends without a solution hard-fixes ("decimates", "pins") the most reliable
 * undecided bit, keeps every message and goes on.  For the degenerate, short-cycle graphs of quantum LDPC codes, where
 * plain min-sum stalls: no elimination, no table of random strengths, one parameter (max_decimations).  Like
 * ldpc_minsum_* it has no division and no transcendental function, so THE RULE below has one legal outcome in IEEE
 * binary32 and a numpy model equals the device in every bit.
 *
 * Inputs.  H, channel_llr[n], alpha, clip: as ldpc_minsum_create takes them.  round_iters T >= 0; max_decimations Dmax
 * with 0 <= Dmax <= n; T * (Dmax + 1) at most INT32_MAX; pin = 2.0f * clip must be finite.  A syndrome entry that is not
 * 0 counts as 1.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * State per syndrome: L[j], initially channel_llr[j]; the check-to-bit messages c[i][j], initially +0; the set D of
 * decimated bits, initially empty; a pending bit j*, initially none, with its sign; iters = 0.
 * For t = 1, 2, ...:
 *   1. Check sweep: step 1 of the min-sum rule above on L, unchanged.  A pinned bit enters like any other: because
 *      |c| <= alpha * clip <= clip its b_k is exactly +-clip, which is never < m1, so it gives its sign to par and nothing
 *      to the minima.
 *   2. Bit sweep.  The pending bit, if there is one:  L[j*] = negative ? -pin : +pin, and nothing is pending any more.
 *      For every other j not in D:  L[j] = channel_llr[j] + c[i_0][j] + c[i_1][j] + ... from the left, checks ascending
 *      (the min-sum rule).  For every other j in D, L[j] is not written.  Then err[j] = (L[j] <= 0) and iters = t.
 *   3. Test.  If H * err == syndrome (an empty check is matched only by a 0 entry): converged = 1, the syndrome stops.
 *   4. End of a round, only when t is a multiple of T and the test failed.  If |D| == Dmax (which covers |D| == n):
 *      converged = 0, the syndrome stops.  Otherwise j* = the j not in D with the largest |L[j]|, the lowest j on a tie
 *      (the maximum over (magnitude, -index), so any reduction order is legal); negative = (L[j*] <= 0); j* enters D and
 *      is pending.  The messages are kept.  A bit of degree 0 may be chosen like any other.
 * The order is part of the rule: check sweep t + 1 still reads L[j*] as bit sweep t left it, and the pin stands in L
 * from bit sweep t + 1 on.  (A kernel whose stop test of iteration t rides on check sweep t + 1 therefore decimates
 * between that check sweep and the bit sweep after it, and needs no sweep of its own for the test.)  A syndrome never
 * stops with a bit pending: iteration t + 1 always follows a decimation.
 *
 * Outputs.  errors [batch][n] uint8 = (L <= 0); converged [batch] uint8; llr [batch][n] DOUBLE (may be NULL): L widened
 * exactly, so a pinned bit reads +-pin; iters [batch] int32 (may be NULL); decimated [batch] int32 (may be NULL): |D|
 * when the syndrome stopped.  round_iters = 0: zeros everywhere (converged = 0, llr = 0, iters = 0, decimated = 0), as
 * max_iters = 0 of min-sum.  batch = 0: LDPC_OK, nothing touched.
 *
 * Consequence.  With max_decimations = 0 every output equals ldpc_minsum_* (flooding) with max_iters = round_iters in
 * every bit, and decimated = 0.
 *
 * ldpc_decim_kernel: 1 = on-chip (L, the check records, D and the syndromes of the S <= 64 syndromes a workgroup holds
 * live in LDS for the whole decode; needs (4 (n + record words + ceil(n / 32)) + s) bytes <= 159 KiB for one syndrome,
 * records as in ldpc_minsum_kernel); 2 = unlimited (tiles of 64 syndromes in a workspace the handle owns, sized by the
 * resident workgroups; any H with nnz < 2^28); 0 for NULL.  options->kernel_variant 0 = by size, 1 / 2 force a tier (1
 * where the state does not fit: LDPC_ERR_UNSUPPORTED).  A tile ends with its last syndrome, after at most
 * T * (Dmax + 1) iterations.
 *
 * ldpc_decim_tile_syndromes, ldpc_decim_last_grid: as ldpc_minsum_tile_syndromes and ldpc_minsum_last_grid -- the S of
 * the handle, and the workgroups of its most recent kernel launch (0 before any launch); 0 for NULL.
 *
 * ldpc_decim_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for a NULL or non-finite
 * channel_llr, a negative round_iters, max_decimations outside 0 .. n, round_iters * (max_decimations + 1) beyond
 * INT32_MAX, a clip whose double is not finite, alpha or clip outside their min-sum ranges, a kernel_variant outside
 * 0..2 and a pattern ldpc_bp_create rejects; without a device LDPC_ERR_NO_DEVICE; s, n or nnz of 2^28 or more:
 * LDPC_ERR_UNSUPPORTED.  The decode entries behave as those of ldpc_minsum_*: ldpc_decim_decode_batch takes HOST buffers
 * and is synchronous (its wait is bounded by ldpc_set_wait_limit_ms); ldpc_decim_decode_batch_device takes DEVICE
 * pointers and is asynchronous on `stream`; calls on one handle run in call order whatever streams they are given.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_decim_decoder ldpc_decim_decoder;

/* Optional; pass NULL to ldpc_decim_create for defaults.  A zeroed struct means defaults too, except `device` (0 is
 * device 0; -1 = the current one): alpha = 0 / clip = 0 select 0.75 / 1.0e6f. */
typedef struct ldpc_decim_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the bit-to-check values, finite, > 0, 2 * clip finite; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_decim_kernel */
    int32_t reserved[12];
} ldpc_decim_options;

/* The seven ldpc_decim_* functions are declared in ldpc_mi355x_decim.h, which this header includes here: this file and
 * ldpc_mi355x_debug.h keep the functions they declared before the section was added. */
#include "ldpc_mi355x_decim.h"

/* ------------------------------------------------------------------------
 * Pauli relay min-sum decoder: the joint X/Z (Pauli) min-sum of ldpc_pauli_minsum_* run with the per-qubit MEMORY and the
 * chain of LEGS of ldpc_relay_*, returning the Pauli solution of lowest prior weight among the first `stop_after` it finds.
 * One decoder over both check matrices of a CSS code (three beliefs a qubit, so the correlation a Y error puts between
 * the two sides is used) that also gets out of the stalls of plain min-sum on degenerate graphs.  Not a decoder of the
 * reference.  Like its two parents it has no division and no transcendental function, so THE RULE below has one legal
 * outcome in IEEE binary32 and a numpy model equals the device in every bit, LLRs included.  Flooding schedule only.
 *
 * Inputs.  n, hx (rx >= 1 rows), hz (rz >= 1 rows), prior_x[n], prior_y[n], prior_z[n]: as ldpc_pauli_minsum_create takes
 * them.  legs >= 1; gammas[legs][n] binary32, the memory strengths, each finite with -1 < gamma < 1: one strength per qubit
 * and leg, shared by its three beliefs; leg_iters[legs] int32, each >= 0, their sum at most INT32_MAX; stop_after >= 1
 * (default 1); alpha, clip: as ldpc_minsum_create takes them.  The checks are numbered Hx rows first (0 .. rx - 1), then Hz
 * rows (rx .. rx + rz - 1).  Syndromes sx [batch][rx] (= Hx ez) and sz [batch][rz] (= Hz ex); an entry that is not 0 counts
 * as 1.  The library draws no random number and calls no log: the caller supplies priors and gammas.
 *
 * THE RULE.  All arithmetic is binary32, every operation rounded once (no fused multiply-add), subnormals kept.
 * min(x, y) below means  x < y ? x : y  with the operands in the order given.
 * Derived once per handle, for W = X, Y, Z:
 *   g0W[r][j] = (1.0f - gammas[r][j]) * prior_W[j]                       (one subtraction, one multiplication)
 *   qW[j]     = (int64) rint(clamp((double) prior_W[j], -2^24, 2^24) * 2^16)        (the product is exact in double)
 * n > 2^22 answers LDPC_ERR_UNSUPPORTED, so a weight (a sum of one q per qubit) always fits int64.
 * State per syndrome: the posteriors MX[j], MY[j], MZ[j], initially prior_x[j], prior_y[j], prior_z[j]; the totals TX[j],
 * TZ[j]; the check-to-qubit messages c[i][j]; found = 0, iters = 0; best, a Pauli pattern, and its weight best_w.
 * For leg r = 0 .. legs - 1 (a leg with leg_iters[r] = 0 is skipped):
 *   Leg start.  Every c <- +0;  every TX[j], TZ[j] <- +0.
 *   Derived wherever read, with the M that stands at that moment:
 *     LambdaW[j] = g0W[r][j] + gammas[r][j] * MW[j]   (multiply, then add)   for W = X, Y, Z;
 *     GX[j] = LambdaX[j] + TX[j];   GZ[j] = LambdaZ[j] + TZ[j];   GY[j] = (LambdaY[j] + TX[j]) + TZ[j].
 *   For t = 1 .. leg_iters[r]:
 *     1. Check sweep: step 1 of THE RULE of ldpc_pauli_minsum_* on these G, verbatim -- u_k and w_k by the kind of row,
 *        b_k = min(max((u_k - c[i][j_k]) - w_k, -clip), clip), the ascending scan for m1, m2, a, par from the check's own
 *        syndrome entry, the new message alpha * (k == a ? m2 : m1) with its sign bit set iff par XOR neg_k (-0 included);
 *        all b_k of a check are formed from the old state; a check with no qubits sends nothing.
 *     2. Bit sweep, for every j.  The new TX[j] = ((+0 + c[i_0][j]) + c[i_1][j]) + ... over the Hz checks of j in ascending
 *        order, the new TZ[j] the same sum over the Hx checks of j.  With LambdaW from the OLD M:
 *          MX[j] = LambdaX[j] + TX[j];   MZ[j] = LambdaZ[j] + TZ[j];   MY[j] = (LambdaY[j] + TX[j]) + TZ[j].
 *        (The next check sweep forms its G with LambdaW from this NEW M and the same TX, TZ.)  Decision on (MX, MY, MZ)
 *        exactly as ldpc_pauli_minsum_* decides on (GX, GY, GZ):  best = X, g = MX;  if MZ < g { best = Z, g = MZ };
 *        if MY < g { best = Y, g = MY };  E = (g <= 0) ? best : I;  ex[j] = (E is X or Y);  ez[j] = (E is Z or Y).
 *        iters += 1.
 *     3. Test.  If Hz ex == sz and Hx ez == sx (an empty check is matched only by a 0 entry):  w = the sum over j of
 *        qX[j] where E is X, qY[j] where it is Y, qZ[j] where it is Z, 0 where it is I, in int64 (exact, so any summation
 *        order is legal);  if found == 0 or w < best_w: best = (ex, ez), best_w = w (a tie keeps the earlier solution);
 *        found += 1;  if found == stop_after the syndrome stops, otherwise the leg ends and the next leg starts from
 *        this M.
 *   A leg that uses up leg_iters[r] without a solution ends, and the next starts from its M.
 * After the last leg the syndrome stops.
 *
 * Outputs.  gx [batch][n] uint8 and gz [batch][n] uint8: the X part and the Z part of best if found > 0, else the decision
 * on (MX, MY, MZ) as they stand; converged [batch] uint8 = (found > 0); iters [batch] int32 (may be NULL): the total over
 * all legs; solutions [batch] int32 (may be NULL) = found; llr [batch][3][n] DOUBLE (may be NULL): the planes MX, MY, MZ as
 * they stand when the syndrome stops, widened exactly -- with found > 1 that is the M of the LAST solution (or of the last
 * iteration), not necessarily the M of `best`.  Every leg of 0 iterations: zeros everywhere (converged = 0, llr = 0,
 * iters = 0, solutions = 0).  batch = 0: LDPC_OK, nothing touched.
 *
 * Consequence.  With legs = 1, gammas all 0, stop_after = 1 and no prior equal to -0, every output equals
 * ldpc_pauli_minsum_* with max_iters = leg_iters[0] in every bit, the LLR planes included:  (1 - 0) * p = p,
 * p + (+-0) = p, so LambdaW = prior_W and M is the G of that rule after every bit sweep.
 *
 * ldpc_pauli_relay_kernel: 1 = on-chip (the state of the S <= 64 syndromes a workgroup holds lives in LDS for the whole
 * decode: the three G the check sweep reads, MX, MY, MZ, the check records of both sides, a bit plane each for the X part
 * and the Z part of best, the syndromes; needs (4 (6 n + record words + 2 ceil(n / 32)) + rx + rz) bytes <= 159 KiB for
 * one syndrome, records as in ldpc_minsum_kernel); 2 = unlimited (tiles of 64 syndromes in a workspace the handle owns,
 * sized by the resident workgroups); 0 for NULL.  options->kernel_variant 0 = by size, 1 / 2 force a tier (1 where the
 * state does not fit: LDPC_ERR_UNSUPPORTED).  ldpc_pauli_relay_tile_syndromes and ldpc_pauli_relay_last_grid: as
 * ldpc_minsum_tile_syndromes and ldpc_minsum_last_grid, by the same policy over that state.  A tile ends with its last
 * syndrome.
 *
 * ldpc_pauli_relay_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work -- for everything
 * ldpc_pauli_minsum_create and ldpc_relay_create refuse: a NULL or non-finite prior, a NULL gammas or leg_iters, a gamma
 * that is not finite or outside (-1, 1), legs < 1, a negative leg_iters entry, a leg_iters sum beyond INT32_MAX,
 * stop_after < 0 (0 = default 1), alpha outside (0, 1], clip not in (0, inf), a kernel_variant outside 0..2, a NULL pattern
 * or one ldpc_bp_create rejects on either side, and rx < 1 or rz < 1; without a device LDPC_ERR_NO_DEVICE.  The library
 * does not check that Hx and Hz commute.  The decode entries reject a NULL handle, a negative batch and a NULL required
 * pointer the same way.  ldpc_pauli_relay_decode_batch takes HOST buffers and is synchronous (its wait is bounded by
 * ldpc_set_wait_limit_ms); ldpc_pauli_relay_decode_batch_device takes DEVICE pointers and is asynchronous on `stream`;
 * calls on one handle run in call order whatever streams they are given.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_pauli_relay_decoder ldpc_pauli_relay_decoder;

/* Optional; pass NULL to ldpc_pauli_relay_create for defaults.  A zeroed struct means defaults too, except `device` (0 is
 * device 0; -1 = the current one): alpha = 0 / clip = 0 / stop_after = 0 select 0.75 / 1.0e6f / 1. */
typedef struct ldpc_pauli_relay_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    float alpha;             /* normalisation factor in (0, 1]; 0 = default 0.75 */
    float clip;              /* clamp of the qubit-to-check values, finite, > 0; 0 = default 1.0e6f */
    int32_t kernel_variant;  /* 0 = auto; 1, 2 force that tier of ldpc_pauli_relay_kernel */
    int32_t stop_after;      /* solutions to collect before a syndrome stops; 0 = default 1 */
    int32_t reserved[11];
} ldpc_pauli_relay_options;

/* The seven ldpc_pauli_relay_* functions are declared in ldpc_mi355x_pauli_relay.h, which this header includes here: this
 * file and ldpc_mi355x_debug.h keep the functions they declared before the section was added. */
#include "ldpc_mi355x_pauli_relay.h"

/* ------------------------------------------------------------------------
 * Joint Pauli min-sum decoder of a general (non-CSS) stabilizer code, whose checks may mix Pauli types: the rule of
 * ldpc_pauli_minsum_* with a Pauli type per edge and three message totals per qubit.  THE RULE, the options struct, every
 * status and the seven ldpc_stab_minsum_* functions are stated in ldpc_mi355x_stab.h, which this header includes here.
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
#include "ldpc_mi355x_stab.h"

/* ------------------------------------------------------------------------
 * Sliding-window decoding: the step between two windows.  A model H (D detectors x N mechanisms, zero-based CSC) too
 * long to decode in one piece is decoded window by window: window k sees the detectors det_k and the mechanisms mech_k,
 * any decoder of this library decodes its syndromes against H[det_k, mech_k], the first mechanisms of its guess --
 * commit_k, positions in mech_k -- are kept for good, their effect is XORed into the RESIDUAL syndrome (which starts as a
 * copy of the syndromes), and the next window reads its syndromes out of the residual.  A handle holds K windows, given
 * as three lists of lists (ptr[K + 1], idx[ptr[K]]): det_k = det_idx[det_ptr[k] .. det_ptr[k + 1]) and so on.  Which
 * windows a model is cut into is the caller's business (the Python layer's window_plan does it by detector layers);
 * this section only requires what makes the step well defined.
 *
 * Layouts as everywhere in this header: residual [batch][D], guess [batch][N], win_syndromes [batch][|det_k|],
 * win_guess [batch][|mech_k|], next_syndromes [batch][|det_{k+1}|], conv and win_conv [batch], all uint8.  Entries are
 * read by their low bit (flags: by "not 0"), and every entry written is 0 or 1.  The arrays of a call must not overlap.
 *
 * THE RULE, per column i of the call.
 *   gather(k):   win_syndromes(i, r) = residual(i, det_k[r]) & 1.                      Nothing else is touched.
 *   commit(k):
 *     - for c in commit_k:  guess(i, mech_k[c]) = win_guess(i, c) & 1;
 *     - for every detector d that has a stored entry in a committed column, i.e. (d, mech_k[c]) is stored in H for some
 *       c in commit_k:  residual(i, d) = (residual(i, d) & 1) ^ XOR over those c of (win_guess(i, c) & 1).  The FULL
 *       column of H counts, also its detectors outside det_k;
 *     - where d_win_conv and d_conv are both given:  conv(i) = (k == 0 ? 1 : conv(i) != 0) & (win_conv(i) != 0);
 *     - where d_next_syndromes is given:  next_syndromes(i, r) = the NEW residual(i, det_{k+1}[r]) & 1 -- gather(k + 1)
 *       fused into the step;
 *     - every other entry of residual and guess keeps its value.
 *   Consequence: if every mechanism with a stored entry is committed by exactly one window, the windows are committed
 *   in order 0 .. K - 1 on a residual that started as the syndromes, and guess is zero where no window commits, then
 *   after the last commit residual = (syndromes & 1) ^ H * guess in every detector that H touches.
 *
 * ldpc_windows_create answers LDPC_ERR_INVALID_ARGUMENT -- before any device work, with a message that names the window
 * and the index -- for a pattern ldpc_bp_create rejects, a NULL list, a ptr array that does not start at 0 or falls, an
 * index out of range (det_idx in [0, D), mech_idx in [0, N), commit_idx in [0, |mech_k|)), a list that is not ascending
 * and distinct, and a mechanism committed by two windows; D, N, nnz or K of 2^28 or more: LDPC_ERR_UNSUPPORTED; without
 * a device LDPC_ERR_NO_DEVICE.  The tables are built once, on the host, and live in device memory as 32-bit indices.
 * The two steps answer LDPC_ERR_INVALID_ARGUMENT for a NULL handle, k outside [0, K), a negative batch,
 * d_next_syndromes with k = K - 1, and a NULL required pointer (d_win_conv, d_conv and d_next_syndromes are optional).
 * batch = 0: LDPC_OK, nothing touched.  Both take DEVICE pointers and are asynchronous on `stream`; calls on one handle
 * run in call order whatever streams they are given.  ldpc_windows_destroy waits for the device (bounded by
 * ldpc_set_wait_limit_ms).  ldpc_windows_count: K; 0 for NULL.
 *
 * Added WITHOUT a change of LDPC_MI355X_ABI_VERSION (symbols only): detect them by symbol lookup.
 * ------------------------------------------------------------------------ */
typedef struct ldpc_windows ldpc_windows;

/* Optional; pass NULL to ldpc_windows_create for defaults (current device). */
typedef struct ldpc_windows_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t reserved[15];
} ldpc_windows_options;

ldpc_status ldpc_windows_create(int64_t D, int64_t N, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                                int64_t K, const int64_t *det_ptr, const int64_t *det_idx,
                                const int64_t *mech_ptr, const int64_t *mech_idx,
                                const int64_t *commit_ptr, const int64_t *commit_idx,   /* positions in the window's mech list */
                                const ldpc_windows_options *options, ldpc_windows **out);
ldpc_status ldpc_windows_destroy(ldpc_windows *w);
int64_t ldpc_windows_count(const ldpc_windows *w);
ldpc_status ldpc_windows_gather_device(ldpc_windows *w, int64_t k, int64_t batch, const uint8_t *d_residual,
                                       uint8_t *d_win_syndromes, void *stream);
ldpc_status ldpc_windows_commit_device(ldpc_windows *w, int64_t k, int64_t batch, const uint8_t *d_win_guess,
                                       const uint8_t *d_win_conv, uint8_t *d_residual, uint8_t *d_guess,
                                       uint8_t *d_conv, uint8_t *d_next_syndromes, void *stream);

/* Diagnostics: 100 MHz ticks spent in {check sweep, variable sweep, convergence test}
 * of that call, summed over workgroups (one sampling wave each). */
ldpc_status ldpc_bp_call_phase_ticks(ldpc_bp_decoder *dec, int32_t calls_back, uint64_t ticks[3]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_MI355X_H */
