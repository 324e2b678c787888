"""The tier and the tile width of the min-sum and the relay decoder without a GPU: ldpc_debug_tile_plan (the function both
`create` routines call, csrc/tile_plan.hpp) against the rule restated here from the comments of the kernel headers --
never by calling the library for the sizes:

    a tile of S syndromes holds  S (4 (n + rec_words) + s)  bytes (min-sum),
                                 S (4 (2 n + rec_words + ceil(n / 32)) + s)  bytes (relay), rounded up to 256;
    S = the largest power of two <= 64 whose state fits 79 KiB (two workgroups a CU), else the largest that fits 159 KiB,
    else the unlimited tier with S = 64.

tests/test_gpu_minsum_tiles.py runs every row of TABLE on the device and asserts the width read back from the handle;
tests/test_gpu_family_widths.py does the same for PAULI_TABLE and PRIORS_TABLE (the Pauli decoder and the entries with
per-syndrome priors, whose states have other sizes: ldpc_debug_pauli_tile_plan, ldpc_debug_priors_tile_plan).
At the end: the builder of the check records (ms_records, the same header) under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc

OK, INVALID, UNSUPPORTED = 0, 1, 5
KIB79, KIB159 = 79 * 1024, 159 * 1024

# (3,6)-regular shapes, s = n / 2, rec_words = 4 s: n -> ((tier, S) of min-sum, (tier, S) of relay)
TABLE = {
    96: ((1, 64), (1, 32)),
    192: ((1, 32), (1, 16)),
    384: ((1, 16), (1, 8)),
    768: ((1, 8), (1, 4)),
    1536: ((1, 4), (1, 2)),
    3072: ((1, 2), (1, 1)),
    6144: ((1, 1), (1, 1)),       # min-sum inside the 79 KiB budget, relay inside the 159 KiB one
    12288: ((1, 1), (2, 64)),     # min-sum inside the 159 KiB budget
    13824: ((2, 64), (2, 64)),
}


def state_bytes(s, n, rec_words, S, relay):
    words = 2 * n + rec_words + (n + 31) // 32 if relay else n + rec_words
    return ((4 * words + s) * S + 255) // 256 * 256


def rule(s, n, rec_words, relay, variant=0):
    """(tier, S) by the rule, or None where variant 1 finds no fit."""
    S = 0
    for budget in (KIB79, KIB159):
        fits = [w for w in (64, 32, 16, 8, 4, 2, 1) if state_bytes(s, n, rec_words, w, relay) <= budget]
        if fits:
            S = fits[0]
            break
    if variant == 1:
        return (1, S) if S else None
    if variant == 2:
        return (2, 64)
    return (1, S) if S else (2, 64)


def plan(s, n, rec_words, relay, variant=0, experiments=False):
    """(status, tier, S, state bytes) of ldpc_debug_tile_plan."""
    L = ldpc._capi.lib(experiments)
    tier, S, nbytes = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int64(-7)
    st = L.ldpc_debug_tile_plan(s, n, rec_words, int(relay), variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(nbytes))
    return st, tier.value, S.value, nbytes.value


def record_words(H):
    deg = np.diff(sp.csr_matrix(H).indptr)
    return int(sum(0 if d == 0 else 4 if d <= 32 else 5 if d <= 64 else d for d in deg))


def shape_for(target, relay):
    """(s, n) with rec_words = 0 whose one-syndrome state is exactly `target` bytes (a multiple of 4) before the rounding."""
    assert target % 4 == 0
    n = target // 4
    while 4 * ((2 * n + (n + 31) // 32) if relay else n) > target:
        n -= 1
    s = target - 4 * ((2 * n + (n + 31) // 32) if relay else n)
    assert (4 * ((2 * n + (n + 31) // 32) if relay else n) + s) == target and s % 4 == 0
    return s, n


def test_per_lane_bytes_of_the_table_shapes():
    """12.5 n bytes a syndrome for min-sum and 16.625 n for relay: what the table's widths follow from."""
    for n in TABLE:
        assert state_bytes(n // 2, n, 2 * n, 1, False) == -(-int(12.5 * n) // 256) * 256
        assert state_bytes(n // 2, n, 2 * n, 1, True) == -(-int(16.625 * n) // 256) * 256


@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
@pytest.mark.parametrize("n", sorted(TABLE))
def test_the_table(n, relay):
    s, rec = n // 2, 2 * n
    want = TABLE[n][int(relay)]
    assert rule(s, n, rec, relay) == want          # the table follows from the restated rule
    for experiments in (False, True):
        st, tier, S, nbytes = plan(s, n, rec, relay, experiments=experiments)
        assert (st, tier, S) == (OK, *want)
        assert nbytes == state_bytes(s, n, rec, S, relay)
        if tier == 1:
            assert nbytes <= KIB159 and (S == 64 or state_bytes(s, n, rec, 2 * S, relay) > KIB79)
    # which budget the last on-chip rows fit
    if n == 6144:
        assert state_bytes(s, n, rec, 1, False) <= KIB79 < state_bytes(s, n, rec, 1, True) <= KIB159
    if n == 12288:
        assert KIB79 < state_bytes(s, n, rec, 1, False) <= KIB159 < state_bytes(s, n, rec, 1, True)
    if n == 13824:
        assert state_bytes(s, n, rec, 1, False) > KIB159


def test_the_shapes_of_the_existing_gpu_tests_keep_their_tiers():
    """BB-72 H_X, the (240, 8, 4) code and the 150-bit irregular graph of tests/test_gpu_minsum.py / test_gpu_relay.py: tier 1
    by size for all of them (those tests assert the tier), at S = 64, 16 and 32."""
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    Hx = sp.csc_matrix(np.asarray(Hx, dtype=np.uint8))
    assert Hx.shape == (36, 72) and record_words(Hx) == 144
    for relay in (False, True):
        assert plan(36, 72, 144, relay)[:3] == (OK, 1, 64)
        assert plan(36, 72, 144, relay, 2)[:3] == (OK, 2, 64)
    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    assert H.shape == (120, 240) and record_words(H) == 480
    for relay in (False, True):
        assert plan(120, 240, 480, relay)[:3] == (OK, 1, 16) and plan(120, 240, 480, relay, 1)[:3] == (OK, 1, 16)
    # the irregular graph: 27 checks of degree 0, 1, 33, 64, 70 and 22 of degree 3 ... 6 (its builder asserts them), 150 bits
    rec = 0 + 4 + 5 + 5 + 70 + 22 * 4
    for relay in (False, True):
        assert plan(27, 150, rec, relay)[:3] == (OK, 1, 32) and plan(27, 150, rec, relay, 1)[:3] == (OK, 1, 32)


# ---- the shapes of tests/test_gpu_family_widths.py --------------------------------------------------------------------
# Pauli, Hx and Hz both (3,6)-regular over n qubits: s = n checks, rec_words = 4 n, 4 (2 n + 4 n) + n = 25 n bytes a syndrome.
# n -> (tier, S)
PAULI_TABLE = {
    48: (1, 64),
    96: (1, 32),
    192: (1, 16),
    384: (1, 8),
    768: (1, 4),
    1536: (1, 2),
    3072: (1, 1),       # inside the 79 KiB budget
    6144: (1, 1),       # inside the 159 KiB budget
    6912: (2, 64),      # 172,800 bytes a syndrome: the unlimited tier by size
}
# The flooding entries with per-syndrome priors, (3,6)-regular H: 12.5 n bytes of plain state and 4 n of priors, 16.5 n a
# syndrome.  `extra`: one more check row of degree 33 (a five-word record), which makes s odd, so that s S is no multiple of
# 4 and the priors block starts behind padding bytes.  (n, extra) -> ((tier, S) of the priors entries, (tier, S) of the plain)
PRIORS_TABLE = {
    (72, 0): ((1, 64), (1, 64)),
    (192, 0): ((1, 16), (1, 32)),
    (384, 0): ((1, 8), (1, 16)),
    (768, 0): ((1, 4), (1, 8)),
    (1536, 0): ((1, 2), (1, 4)),
    (1536, 1): ((1, 2), (1, 4)),      # s = 769: s S % 4 == 2
    (3072, 0): ((1, 1), (1, 2)),
    (3072, 1): ((1, 1), (1, 2)),      # s = 1537: s S % 4 == 1
    (6144, 0): ((1, 1), (1, 1)),      # the priors entries inside the 159 KiB budget, the plain ones inside the 79 KiB one
}


def priors_state_bytes(s, n, rec_words, S):
    """The plain blocks, the next word boundary, then P [n][S] f32 (minsum_kernels.hpp); rounded up to 256."""
    return (((4 * (n + rec_words) + s) * S + 3) // 4 * 4 + 4 * n * S + 255) // 256 * 256


def widest_fit(size_of):
    """(tier, S) by the rule of the module docstring for a state of size_of(S) bytes."""
    for budget in (KIB79, KIB159):
        fits = [w for w in (64, 32, 16, 8, 4, 2, 1) if size_of(w) <= budget]
        if fits:
            return 1, fits[0]
    return 2, 64


def debug_plan(name, *args, experiments=False):
    """(status, tier, S, state bytes) of one of the ldpc_debug_*_tile_plan functions."""
    tier, S, nbytes = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int64(-7)
    st = getattr(ldpc._capi.lib(experiments), name)(*args, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(nbytes))
    return st, tier.value, S.value, nbytes.value


@pytest.mark.parametrize("experiments", [False, True])
def test_the_shapes_of_the_family_width_tests_keep_their_rows(experiments):
    """tests/test_gpu_family_widths.py asserts these widths on the handles; a planner change that moves a shape off its row
    fails here first."""
    for n, want in PAULI_TABLE.items():
        size_of = lambda S: (25 * n * S + 255) // 256 * 256   # noqa: E731
        assert 4 * (2 * n + 4 * n) + n == 25 * n and widest_fit(size_of) == want, n
        assert debug_plan("ldpc_debug_pauli_tile_plan", n, n, 4 * n, 0, experiments=experiments) == (OK, *want, size_of(want[1])), n
        on_chip = debug_plan("ldpc_debug_pauli_tile_plan", n, n, 4 * n, 1, experiments=experiments)
        assert on_chip[:3] == (OK, *want) if want[0] == 1 else on_chip[0] == UNSUPPORTED, n
    assert 25 * 3072 <= KIB79 < 25 * 6144 <= KIB159 < 25 * 6912
    for (n, extra), (want_priors, want_plain) in PRIORS_TABLE.items():
        s, rec = n // 2 + extra, 2 * n + 5 * extra
        assert widest_fit(lambda S: priors_state_bytes(s, n, rec, S)) == want_priors, (n, extra)
        assert widest_fit(lambda S: state_bytes(s, n, rec, S, False)) == want_plain, (n, extra)
        S = want_priors[1]
        assert debug_plan("ldpc_debug_priors_tile_plan", s, n, rec, 0, 0, experiments=experiments) == (OK, *want_priors, priors_state_bytes(s, n, rec, S))
        assert debug_plan("ldpc_debug_tile_plan", s, n, rec, 0, 0, experiments=experiments)[:3] == (OK, *want_plain)
        # a layered handle keeps no priors block: its priors plan is its plain plan
        assert debug_plan("ldpc_debug_priors_tile_plan", s, n, rec, 1, 0, experiments=experiments)[:3] == (OK, *want_plain)
        assert ((s * S) % 4 != 0) == bool(extra), (n, extra)
    assert (769 * 2) % 4 == 2 and 1537 % 4 == 1 and 3072 % 4 == 0
    assert priors_state_bytes(3072, 6144, 12288, 1) > KIB79 >= state_bytes(3072, 6144, 12288, 1, False)


@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
def test_the_boundaries_of_both_budgets(relay):
    """rec_words = 0 and n, s free: one syndrome of exactly 79 KiB, 4 bytes more, exactly 159 KiB, 4 bytes more."""
    s, n = shape_for(KIB79, relay)
    assert state_bytes(s, n, 0, 1, relay) == KIB79
    assert plan(s, n, 0, relay) == (OK, 1, 1, KIB79)
    s, n = shape_for(KIB79 + 4, relay)
    assert state_bytes(s, n, 0, 1, relay) == KIB79 + 256            # rounded up: beyond the budget of two workgroups a CU
    # ... and two such syndromes still fit the budget of one: the 159 KiB budget takes its own largest S, not 1
    assert state_bytes(s, n, 0, 2, relay) <= KIB159 < state_bytes(s, n, 0, 4, relay)
    assert plan(s, n, 0, relay) == (OK, 1, 2, state_bytes(s, n, 0, 2, relay))
    s, n = shape_for(KIB159 // 2, relay)                              # the last size of that window, and the first beyond it
    assert state_bytes(s, n, 0, 2, relay) == KIB159 and plan(s, n, 0, relay) == (OK, 1, 2, KIB159)
    s, n = shape_for(KIB159 // 2 + 4, relay)
    assert state_bytes(s, n, 0, 2, relay) == KIB159 + 256 and plan(s, n, 0, relay)[:3] == (OK, 1, 1)
    s, n = shape_for(KIB159, relay)
    assert state_bytes(s, n, 0, 1, relay) == KIB159
    assert plan(s, n, 0, relay) == (OK, 1, 1, KIB159) and plan(s, n, 0, relay, 1) == (OK, 1, 1, KIB159)
    s, n = shape_for(KIB159 + 4, relay)
    assert state_bytes(s, n, 0, 1, relay) == KIB159 + 256
    assert plan(s, n, 0, relay) == (OK, 2, 64, state_bytes(s, n, 0, 64, relay))
    assert plan(s, n, 0, relay, 1)[0] == UNSUPPORTED
    assert b"kernel_variant 1" in ldpc._capi.lib().ldpc_last_error()
    assert plan(s, n, 0, relay, 2)[:3] == (OK, 2, 64)


def test_the_window_above_79_kib_a_syndrome_where_two_still_fit_159_kib():
    """(3,6) min-sum at n = 6480: 81,000 bytes a syndrome miss 79 KiB, 2 x 81,000 fit 159 KiB: S = 2, not 1."""
    n = 6480
    assert 4 * (n + 2 * n) + n // 2 == 81000 and KIB79 < 81000 and 2 * 81000 <= KIB159
    assert plan(n // 2, n, 2 * n, False)[:3] == (OK, 1, 2)
    n = 6528                                                   # 81,600 a syndrome: 163,200 > 159 KiB: S = 1
    assert 2 * (4 * 3 * n + n // 2) > KIB159
    assert plan(n // 2, n, 2 * n, False)[:3] == (OK, 1, 1)


@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
def test_forced_variants_and_empty_graphs(relay):
    for n in TABLE:
        s, rec = n // 2, 2 * n
        st, tier, S, nbytes = plan(s, n, rec, relay, 2)
        assert (st, tier, S, nbytes) == (OK, 2, 64, state_bytes(s, n, rec, 64, relay))      # variant 2: always tier 2, S = 64
        want = rule(s, n, rec, relay, 1)
        if want is None:
            assert plan(s, n, rec, relay, 1)[0] == UNSUPPORTED
        else:
            assert plan(s, n, rec, relay, 1)[:3] == (OK, *want) and want == TABLE[n][int(relay)]
    assert rule(6912, 13824, 27648, relay, 1) is None and rule(6144, 12288, 24576, True, 1) is None
    # nothing to decode: no crash, the widest tile
    for s, n in ((0, 0), (0, 5), (3, 0)):
        for variant in (0, 1, 2):
            assert plan(s, n, 0, relay, variant) == (OK, 2 if variant == 2 else 1, 64, state_bytes(s, n, 0, 64, relay))
    assert plan(0, 0, 0, relay)[3] == 0
    # NULL outputs are allowed; what create refuses is refused here
    L = ldpc._capi.lib()
    assert L.ldpc_debug_tile_plan(36, 72, 144, int(relay), 0, None, None, None) == OK
    assert plan(-1, 72, 144, relay)[0] == INVALID and plan(36, -1, 144, relay)[0] == INVALID
    assert plan(36, 72, -1, relay)[0] == INVALID and plan(36, 72, 144, relay, 3)[0] == INVALID
    assert plan(36, 72, 144, relay, -1)[0] == INVALID and plan(1 << 28, 72, 144, relay)[0] == INVALID


def test_random_shapes_follow_the_restated_rule():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(3000):
        n = int(rng.integers(0, 60000))
        s = int(rng.integers(0, n + 2))
        rec = int(rng.integers(0, 5 * s + 1))
        relay = bool(rng.integers(0, 2))
        variant = int(rng.integers(0, 3))
        want = rule(s, n, rec, relay, variant)
        st, tier, S, nbytes = plan(s, n, rec, relay, variant)
        if want is None:
            assert st == UNSUPPORTED
            continue
        assert (st, tier, S, nbytes) == (OK, *want, state_bytes(s, n, rec, S, relay)), (s, n, rec, relay, variant)
        seen.add(want)
    assert seen == {(1, w) for w in (64, 32, 16, 8, 4, 2, 1)} | {(2, 64)}


def test_getters_answer_zero_for_null():
    for experiments in (False, True):
        L = ldpc._capi.lib(experiments)
        assert L.ldpc_minsum_tile_syndromes(None) == 0 and L.ldpc_minsum_last_grid(None) == 0
        assert L.ldpc_relay_tile_syndromes(None) == 0 and L.ldpc_relay_last_grid(None) == 0


def test_check_records_under_sanitizers(tmp_path):
    """csrc/tile_plan.hpp (ms_records: rec_off, edge_rec, edge_pos and the word count that the three create routines
    upload) built with AddressSanitizer + UBSan (CPU only) and driven by tests/native/records_sanitize.cpp."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "records_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-I", os.path.join(root, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(root, "tests", "native", "records_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK ") and "record sets" in out.stdout, out.stdout + out.stderr
