"""The team kernel with message rows ON CHIP against the CPU oracle, deterministically: every rows-on-chip instantiation
of pick_team.hip (check degree 6 ... 10 x bit degree 3 ... 5 x LLRs on / off x register rows on / off = 60) on a graph of
its own, and the edge inputs of test_gpu_parity.py (channel probabilities 0 and 1, decodes that stop after the first
iterations, syndrome entries 2 / 3, ragged batches, a handle used twice) on graphs large enough to HAVE rows on chip.

Small teams get rows on chip on mid-size graphs through the knobs of the experiments build that tools/fuzz_parity.py
uses (LDPC_TEAM_MIN_ROWS=1, LDPC_TEAM_MAX=4); what ran is read back from ldpc_bp_info and asserted, so a test that does
not reach its instantiation FAILS.  Every comparison is against BPOracle on every syndrome and every bit: hard decisions,
converged flags and iteration counts equal, non-finite LLRs equal exactly, finite ones within LLR_CUT_TOL.

Fewer teams than tiles.  The matrix batch is 8 tiles; the plan (team_plan.cpp team_plan_pure()) gives 8 tiles 8 teams
whatever LDPC_TEAM_CACHE_KIB says while register rows are off -- a budget of >= 6.4 slots is `one_round`, a smaller one
fails team_fit()'s first tier (7 whole slots) and lands on its second (one team per XCD) or on one team per tile -- so the
cache budget alone cannot make a team take a second tile in all four instantiations of a pair.  LDPC_TEAM_XCDS=7 can: it
is the seven-XCD plan team_fit() also picks by itself (seven teams of four, one of them takes the ragged eighth tile in
the slot it has just used), and `teams < tiles` is asserted from ldpc_bp_info after every decode."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc_mod
from oracle import BPOracle

pytestmark = pytest.mark.gpu

# LLRs of the default decoder come from the posterior odds cut to their upper 32 bits (within 5e-7 of log(1 / T), include/
# ldpc_mi355x.h); 1e-6 is what tools/fuzz_parity.py holds them to and tighter than test_gpu_parity.py's LLR_TOL = 1e-5
LLR_CUT_TOL = 1e-6
LLR_EXACT_TOL = 1e-9          # llr_exact=True: log(1 / T) itself, two libms apart (the fuzz's bound)

PAIRS = [(dc, dv) for dc in range(6, 11) for dv in range(3, 6)]
# error rates at which the lanes of one tile stop at many different iterations -- found with the CPU oracle alone on exactly
# the inputs of matrix_inputs(); assert_waterfall() holds the ORACLE's output to it
WATERFALL = {(6, 3): 0.080, (6, 4): 0.115, (6, 5): 0.135, (7, 3): 0.065, (7, 4): 0.090, (7, 5): 0.110,
             (8, 3): 0.050, (8, 4): 0.075, (8, 5): 0.090, (9, 3): 0.040, (9, 4): 0.065, (9, 5): 0.075,
             (10, 3): 0.035, (10, 4): 0.055, (10, 5): 0.065}
REGIMES = ("early", "none", "waterfall")    # early exit (per 0.02), nothing converges (0.20), waterfall
B_MATRIX = 485                               # seven full tiles and one of 37 lanes
ITERS = 30
TEAM = 4                                     # LDPC_TEAM_MAX
W, RREGS, RMAX = 8, 32, 312                  # waves a member, register rows a wave, LDS rows a member (bp_team_kernels.hpp)


def regime_per(dc, dv, regime):
    return {"early": 0.02, "none": 0.20, "waterfall": WATERFALL[(dc, dv)]}[regime]


@functools.lru_cache(maxsize=None)
def regular_graph(dc, dv):
    return ldpc_mod.codes.parity_check_csc(300 * dc, dc, dv)


@functools.lru_cache(maxsize=None)
def matrix_inputs(dc, dv, per):
    H = regular_graph(dc, dv)
    return ldpc_mod.codes.syndromes_of(H, ldpc_mod.codes.random_errors(H.shape[1], B_MATRIX, per, seed=1000 * dc + dv))


def oracle_of(H, per, iters, syn):
    return BPOracle(csc=(H.indptr, H.indices), shape=H.shape, per=per, max_iters=iters).batchdecode(syn, want_llr=True)


@functools.lru_cache(maxsize=None)
def matrix_oracle(dc, dv, per):
    return oracle_of(regular_graph(dc, dv), per, ITERS, matrix_inputs(dc, dv, per))


def assert_waterfall(oconv, oits):
    """A condition on the INPUTS, from the oracle's output only (no device): the leg is a waterfall -- a changed generator
    must not quietly turn it into a second early-exit leg."""
    share, distinct = float(np.mean(oconv)), len(np.unique(oits))
    assert 0.25 <= share <= 0.75 and distinct >= 15, (share, distinct)


def assert_equals_oracle(got, ref, tol, tag):
    """Everything, on every syndrome and every bit.  got / ref = (err, conv, llr | None, its)."""
    err, conv, llr, its = got
    oerr, oconv, ollr, oits = ref
    assert conv.shape == oconv.shape and err.shape == oerr.shape, tag
    assert np.array_equal(conv, oconv), f"{tag}: converged flags differ at {np.flatnonzero(conv != oconv)[:10]}"
    assert np.array_equal(its, oits), f"{tag}: iteration counts differ at {np.flatnonzero(its != oits)[:10]}"
    assert np.array_equal(err, oerr), f"{tag}: hard decisions differ in syndromes {np.unique(np.nonzero(err != oerr)[0])[:10]}"
    if llr is not None:
        fin = np.isfinite(ollr)
        assert np.array_equal(np.isfinite(llr), fin), f"{tag}: finite / non-finite LLRs differ"
        assert np.array_equal(llr[~fin], ollr[~fin], equal_nan=True), f"{tag}: non-finite LLRs differ"
        worst = float(np.max(np.abs(llr[fin] - ollr[fin]))) if fin.any() else 0.0
        print(f"{tag}: worst finite LLR difference {worst:.3e}, non-finite {int((~fin).sum())}")
        assert worst <= tol, f"{tag}: LLRs differ by {worst:.3e} > {tol}"


def planned_rows(H, members, regs):
    """(LDS rows of the fullest member, rows in LDS in all, rows in registers in all) of the host tables for teams of
    `members`, through ldpc_debug_team_rows with the default three static quarters (no device needed)."""
    s, n = H.shape
    colptr = np.ascontiguousarray(H.indptr, dtype=np.int64)
    rowval = np.ascontiguousarray(H.indices, dtype=np.int64)
    deg = (ctypes.c_int32 * 2)()
    shape = (ctypes.c_int32 * 5)()
    vtab = np.zeros((n, 16), dtype=np.int32)
    ctab = np.zeros((s, 4), dtype=np.int32)
    lds_edge = np.full(members * RMAX, -7, dtype=np.int32)
    reg_edge = np.full(members * W * RREGS, -7, dtype=np.int32)
    L = ldpc_mod._capi.lib()
    ldpc_mod._capi.check(L.ldpc_debug_team_rows(s, n, colptr.ctypes.data, rowval.ctypes.data, members, regs, 3, ctypes.byref(deg),
                                                ctypes.byref(shape), vtab.ctypes.data, ctab.ctypes.data, lds_edge.ctypes.data,
                                                reg_edge.ctypes.data), L)
    R, regs_eff = shape[1], shape[4]
    return R, int((lds_edge[: members * R] >= 0).sum()), int((reg_edge[: members * W * max(regs_eff, 1)] >= 0).sum())


def set_team_knobs(monkeypatch, regs, **extra):
    """Small teams with rows on chip on a mid-size graph.  Read when the decoder is created; setting any of them selects
    the experiments build."""
    knobs = {"LDPC_TEAM_MIN_ROWS": "1", "LDPC_TEAM_MAX": str(TEAM), "LDPC_TEAM_REGS": str(regs)}
    knobs.update(extra)
    for k, v in knobs.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def assert_rows_on_chip_ran(info, regs, H=None, tiles=None, tag=""):
    """The intended code ran: the team kernel, teams of four, rows in LDS, and rows in registers exactly when asked for."""
    seen = (info.last_kernel, info.last_team_size, info.last_lds_rows, info.last_rows_on_chip, info.resident_tiles)
    assert info.last_kernel == 4 and info.last_team_size == TEAM and info.last_lds_rows > 0, (tag, seen)
    if regs:
        assert info.last_rows_on_chip > info.last_team_size * info.last_lds_rows, (tag, seen)
    else:
        assert 0 < info.last_rows_on_chip <= info.last_team_size * info.last_lds_rows, (tag, seen)
    if H is not None:       # the plan of ldpc_debug_team_rows for the same members / register rows is the one that ran
        R, in_lds, in_regs = planned_rows(H, TEAM, regs)
        assert (info.last_lds_rows, info.last_rows_on_chip) == (R, in_lds + in_regs), (tag, seen, R, in_lds, in_regs)
        assert in_lds > 0 and (in_regs > 0) == bool(regs) and in_lds + in_regs < H.nnz, (tag, in_lds, in_regs)   # all three homes of a row
    if tiles is not None:   # persistent teams: fewer teams than tiles, somebody takes a second tile in its slot
        assert info.resident_tiles % info.last_team_size == 0 and info.resident_tiles // info.last_team_size < tiles, (tag, seen)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every rows-on-chip instantiation
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regs", [32, 0], ids=["regs32", "regs0"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dc,dv", PAIRS, ids=[f"dc{dc}_dv{dv}" for dc, dv in PAIRS])
def test_rows_on_chip_instantiation_against_the_oracle(ldpc, gpu, monkeypatch, dc, dv, regime, regs):
    """One (check degree, bit degree) pair, one regime, register rows on or off: n = 300 dc, 485 syndromes (seven full tiles
    and one of 37 lanes) on seven persistent teams of four, 30 iterations.  With LLRs and without (the two instantiations),
    everything against the oracle on all 485 syndromes.  On the waterfall leg also through the forced hand-off (rows on
    chip written back, stragglers resumed by the bucket kernels: LDPC_DEFER_T0=48, LDPC_DEFER_T1=16,
    LDPC_NODE_TAKE_MAX=8) and, with register rows, with exact LLRs to 1e-9."""
    H = regular_graph(dc, dv)
    per = regime_per(dc, dv, regime)
    syn = matrix_inputs(dc, dv, per)
    ref = matrix_oracle(dc, dv, per)
    if regime == "waterfall":
        assert_waterfall(ref[1], ref[3])
    elif regime == "early":
        assert ref[1].all()
    else:
        assert not ref[1].any() and (ref[3] == ITERS).all()
    tiles = (B_MATRIX + 63) // 64
    tag = f"({dc},{dv}) {regime} regs {regs}"

    def run(label, tol=LLR_CUT_TOL, **kw):
        dec = ldpc.BeliefPropagationDecoder(H, per, ITERS, kernel_variant=4, **kw)
        for want_llr in (True, False):
            got = dec.decode_batch_host(syn, want_llr=want_llr, want_iters=True)
            info = dec.info()
            print(f"{tag} {label} llr {want_llr}: team {info.last_team_size} lds_rows {info.last_lds_rows} on_chip {info.last_rows_on_chip} "
                  f"workgroups {info.resident_tiles}")
            assert_rows_on_chip_ran(info, regs, H, tiles, f"{tag} {label}")
            assert_equals_oracle(got, ref, tol, f"{tag} {label} llr {want_llr}")
        dec.close()

    set_team_knobs(monkeypatch, regs, LDPC_TEAM_XCDS="7")
    run("plain")
    if regime == "waterfall":
        if regs:
            run("exact", tol=LLR_EXACT_TOL, llr_exact=True)
        set_team_knobs(monkeypatch, regs, LDPC_TEAM_XCDS="7", LDPC_DEFER_T0="48", LDPC_DEFER_T1="16", LDPC_NODE_TAKE_MAX="8")
        run("hand-off")


# ---------------------------------------------------------------------------------------------------------------------
# 2. edge inputs on the on-chip paths
# ---------------------------------------------------------------------------------------------------------------------

def _irregular(n, s, seed, bit_deg_max, check_cap, heavy):
    """Bits of degree 2 ... bit_deg_max on random checks of at most check_cap edges (like _irregular_graph of
    test_gpu_full_size.py, with the cap); heavy: five checks grown to 17 ... 32 edges and check 7 to exactly 34 (beyond every
    register bucket: the O(deg^2) path -- 34, not 40: team_irr_dc_bucket() keeps whole checks in LDS only while such
    checks cost at most nnz / 8 in deg^2)."""
    rng = np.random.default_rng(seed)
    deg = np.zeros(s, dtype=np.int64)
    member = [set() for _ in range(s)]
    for j in range(n):
        for i in rng.choice(np.flatnonzero(deg < check_cap), int(rng.integers(2, bit_deg_max + 1)), replace=False):
            member[int(i)].add(j)
            deg[i] += 1
    if heavy:
        grow = [(int(i), 20) for i in rng.choice(np.setdiff1d(np.arange(s), [7]), 5, replace=False)] + [(7, 34)]
        for i, want in grow:
            free = np.setdiff1d(np.arange(n), sorted(member[i]))
            member[i].update(int(j) for j in rng.choice(free, want - len(member[i]), replace=False))
    rows = [i for i in range(s) for _ in member[i]]
    cols = [j for i in range(s) for j in sorted(member[i])]
    H = sp.csc_matrix((np.ones(len(rows), dtype=np.uint8), (rows, cols)), shape=(s, n))
    H.sort_indices()
    return H


class Host:
    """One way of hosting the on-chip code: graph, knobs, the waterfall rate of the graph, what ldpc_bp_info must say."""

    def __init__(self, name, graph, waterfall, knobs, regs=32):
        self.name, self._graph, self.waterfall, self.knobs, self.regs = name, graph, waterfall, knobs, regs

    @property
    def H(self):
        return self._graph()

    def expect(self, info, B, tag):
        seen = (info.last_kernel, info.last_team_size, info.last_lds_rows, info.last_rows_on_chip, info.resident_tiles)
        tiles = (B + 63) // 64
        assert info.last_kernel == 4, (tag, seen)    # kernel_variant 4 skips the LDS and node kernels, also for B = 1
        if self.name.startswith("R"):
            assert_rows_on_chip_ran(info, self.regs, self.H, None, tag)
        elif self.name == "W":       # two wide teams (one for a single tile) of 8 x per_xcd / 2 members over all XCDs, rows in LDS
            assert info.last_team_size >= 64 and info.resident_tiles == min(2, tiles) * info.last_team_size, (tag, seen)
            assert info.last_lds_rows > 0 and info.last_rows_on_chip > 0, (tag, seen)
        elif self.name.startswith("I"):   # whole checks in the LDS of their owners
            assert info.last_team_size == TEAM and info.last_lds_rows > 0 and info.last_rows_on_chip > 0, (tag, seen)
        else:                        # P: the same teams, every row in the slot
            assert info.last_team_size == TEAM and info.last_lds_rows == 0 and info.last_rows_on_chip == 0, (tag, seen)


@functools.lru_cache(maxsize=None)
def _i8():
    return _irregular(3000, 1500, 8, 4, 8, False)


@functools.lru_cache(maxsize=None)
def _i16():
    return _irregular(3200, 1600, 16, 5, 12, True)


_R_KNOBS = {"LDPC_TEAM_MIN_ROWS": "1", "LDPC_TEAM_MAX": str(TEAM), "LDPC_TEAM_REGS": "32"}
HOSTS = [
    # R: regular graphs of part 1 with register rows: the three table widths / register buckets
    Host("R84", lambda: regular_graph(8, 4), WATERFALL[(8, 4)], _R_KNOBS),
    Host("R105", lambda: regular_graph(10, 5), WATERFALL[(10, 5)], _R_KNOBS),
    Host("R63", lambda: regular_graph(6, 3), WATERFALL[(6, 3)], _R_KNOBS),
    # W: a wide team -- members over all XCDs (release path, LLRs captured in position order); as in the fuzz no LDPC_TEAM_MAX.
    # LDPC_TEAM_SCATTER_TILES=0: the plan deals batches of <= 3 tiles to wide teams too (by default it scatters those
    # WITHOUT rows on chip), so that the small edge batches below run on the code they are meant for
    Host("W", lambda: regular_graph(8, 4), WATERFALL[(8, 4)],
         {"LDPC_TEAM_MIN_ROWS": "1", "LDPC_TEAM_REGS": "32", "LDPC_TEAM_WIDE": "2", "LDPC_TEAM_SCATTER_TILES": "0"}),
    # I: irregular graphs with whole checks in LDS, one per (check, bit) bucket of the IRR instantiations: 8 / 4 and 16 / 16
    Host("I8", _i8, 0.080, _R_KNOBS),
    Host("I16", _i16, 0.080, _R_KNOBS),
    # P: R84 with every row in the slot -- the control that tells a rows-on-chip mistake from a team-kernel one
    Host("P", lambda: regular_graph(8, 4), WATERFALL[(8, 4)], dict(_R_KNOBS, LDPC_TEAM_ROWS="0")),
]
HOST_IDS = [h.name for h in HOSTS]


def test_the_irregular_hosts_have_the_nodes_they_are_for(gpu):
    for H, dc_hi, dv_lo, dv_hi in ((_i8(), 8, 4, 4), (_i16(), 34, 5, 16)):     # (bit degree <= 4: the 4-wide bucket, beyond: the 16-wide)
        cdeg, bdeg = np.diff(H.tocsr().indptr), np.diff(H.indptr)
        assert cdeg.max() == dc_hi and bdeg.min() >= 2 and dv_lo <= bdeg.max() <= dv_hi, (cdeg.max(), bdeg.max())
    cdeg = np.diff(_i16().tocsr().indptr)
    assert int(((cdeg > 16) & (cdeg <= 32)).sum()) == 5 and int((cdeg > 32).sum()) == 1
    for host in HOSTS[4:6]:     # ... and their waterfall rate is one (the regular hosts': part 1)
        H = host.H
        syn = ldpc_mod.codes.syndromes_of(H, ldpc_mod.codes.random_errors(H.shape[1], B_MATRIX, host.waterfall, seed=5))
        _, oconv, _, oits = oracle_of(H, host.waterfall, ITERS, syn)
        assert_waterfall(oconv, oits)


def decode_on_one_handle(ldpc, monkeypatch, host, per, iters, batches, tag):
    """One decoder, the batches one after the other on the SAME handle (stale rows in LDS / registers and stale decision
    words of the double buffer must not leak into the next call), each with LLRs and once more without, each against the
    oracle.  Returns the outputs of the LLR decodes."""
    for k in ("LDPC_TEAM_MAX", "LDPC_TEAM_WIDE", "LDPC_TEAM_SCATTER_TILES", "LDPC_TEAM_ROWS", "LDPC_TEAM_XCDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in host.knobs.items():
        monkeypatch.setenv(k, v)
    H = host.H
    dec = ldpc.BeliefPropagationDecoder(H, per, iters, kernel_variant=4)
    outs = []
    for b, syn in enumerate(batches):
        ref = oracle_of(H, per, iters, syn)
        for want_llr in (True, False):
            got = dec.decode_batch_host(syn, want_llr=want_llr, want_iters=True)
            host.expect(dec.info(), len(syn), f"{tag} batch {b}")
            assert_equals_oracle(got, ref, LLR_CUT_TOL, f"{tag} batch {b} ({len(syn)} syndromes) llr {want_llr}")
            if want_llr:
                outs.append((got, ref))
    dec.close()
    return outs


def errors_syndromes(H, B, per, seed):
    return ldpc_mod.codes.syndromes_of(H, ldpc_mod.codes.random_errors(H.shape[1], B, per, seed=seed))


@pytest.mark.parametrize("per", [0.0, 1e-12, 0.5, 0.999, 1.0])
@pytest.mark.parametrize("host", HOSTS, ids=HOST_IDS)
def test_extreme_channel_probabilities_on_chip(ldpc, gpu, monkeypatch, host, per):
    """per = 0 / 1 give odds 0 / Inf and the NaN reset (belief_propagation.jl:158-160,174-176): 70 random 0/1 syndromes,
    12 iterations, as test_extreme_channel_probabilities -- here where rows live on chip.  At per 0 and 1 the oracle's
    LLRs are +-Inf in bulk, so the exact comparison of the non-finite entries has something to compare."""
    H = host.H
    rng = np.random.default_rng(5)
    syn = rng.integers(0, 2, (70, H.shape[0])).astype(np.uint8)
    other = rng.integers(0, 2, (131, H.shape[0])).astype(np.uint8)
    outs = decode_on_one_handle(ldpc, monkeypatch, host, per, 12, [syn, other], f"{host.name} per {per}")
    if per in (0.0, 1.0):
        assert int((~np.isfinite(outs[0][1][2])).sum()) > syn.shape[0], "the oracle's LLRs should be non-finite in bulk here"


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("host", HOSTS, ids=HOST_IDS)
def test_decodes_that_stop_after_the_first_iterations_on_chip(ldpc, gpu, monkeypatch, host, iters):
    """max_iters 1, 2, 3: on these kernels iteration 1 is bit_update_first (a table of 2 DC entries) and nothing else, 2 and
    3 the first on-chip updates.  At the graph's waterfall rate, at 0.02 and on the all-zero syndrome batch (everything
    converges in iteration 1: the table path alone produces the output)."""
    H = host.H
    for per in (host.waterfall, 0.02):
        zero = np.zeros((B_MATRIX, H.shape[0]), dtype=np.uint8)
        outs = decode_on_one_handle(ldpc, monkeypatch, host, per, iters,
                                    [errors_syndromes(H, B_MATRIX, per, 21), zero, errors_syndromes(H, 200, per, 22)],
                                    f"{host.name} max_iters {iters} per {per}")
        (zerr, zconv, _, zits), _ = outs[1]
        assert zconv.all() and (zits == 1).all() and not zerr.any()


@pytest.mark.parametrize("host", HOSTS, ids=HOST_IDS)
def test_non_binary_syndrome_entries_on_chip(ldpc, gpu, monkeypatch, host):
    """Entries 2 / 3 keep their parity for the sign and can never converge (belief_propagation.jl:136,181): in lanes 0, 1
    and 63 of the first tile and in the last lane of the ragged one, among syndromes that converge."""
    H = host.H
    s = H.shape[0]
    B, iters = 64 + 37, 9
    syn = errors_syndromes(H, B, 0.02, 31).copy()
    marked = [(0, 0, 2), (1, 5, 3), (63, s - 1, 2), (B - 1, 7, 3)]
    for lane, check, value in marked:
        syn[lane, check] = value
    outs = decode_on_one_handle(ldpc, monkeypatch, host, 0.02, iters, [syn, errors_syndromes(H, 70, 0.02, 32)], f"{host.name} entries 2/3")
    (err, conv, llr, its), (oerr, oconv, ollr, oits) = outs[0]
    for lane, _, _ in marked:
        assert not conv[lane] and its[lane] == iters, lane
        # sign as the oracle, wherever the oracle's LLR has one at the precision of the default decoder: its LLRs are the logarithm
        # of the odds cut to their upper 32 bits, within 5e-7 of log(1 / T) (include/ldpc_mi355x.h), so an LLR that the oracle
        # puts at exactly 0 -- odds of 1 behind the NaN reset, a few bits of these lanes -- may come out a cut step (2^-21) to
        # either side.  (NaNs sit where the oracle's do: checked above.)
        num = np.abs(ollr[lane]) > LLR_CUT_TOL
        assert num.sum() >= ollr.shape[1] // 2
        assert np.array_equal(np.sign(llr[lane][num]), np.sign(ollr[lane][num])), lane
    assert conv[2:63].all()      # (the lanes around them are not disturbed)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("host", HOSTS, ids=HOST_IDS)
def test_ragged_batches_on_chip(ldpc, gpu, monkeypatch, host, B):
    """One lane, a tile less one, a full tile, one more, two and a lane -- at the waterfall rate, 30 iterations, then other
    syndromes on the same handle.  (kernel_variant 4 takes the team kernel for B = 1 as well: Host.expect().)"""
    H = host.H
    decode_on_one_handle(ldpc, monkeypatch, host, host.waterfall, ITERS,
                         [errors_syndromes(H, B, host.waterfall, 40 + B), errors_syndromes(H, 100, host.waterfall, 140 + B)],
                         f"{host.name} B {B}")
