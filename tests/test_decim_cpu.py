"""Guided-decimation min-sum decoder without a GPU: the numpy model of the rule (tests/decim_model.py) on a hand-checked
case and on properties that follow from the rule alone, the BB-72 claim the decoder was built for, the argument
validation of ldpc_decim_create (which answers before any device work), the Python constructor's own refusals, the new
symbols, the tile plan (ldpc_debug_decim_tile_plan) against the rule restated here, and the planner addition under the
sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from decim_model import DecimModel
from minsum_model import MinSumModel, llr_of_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5
KIB79, KIB159 = 79 * 1024, 159 * 1024
NEW_SYMBOLS = ("ldpc_decim_create", "ldpc_decim_destroy", "ldpc_decim_kernel", "ldpc_decim_tile_syndromes", "ldpc_decim_last_grid",
               "ldpc_decim_decode_batch", "ldpc_decim_decode_batch_device")


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def bb72():
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx) != 0)


# ---- the model ------------------------------------------------------------------------------------------------------------

def test_model_hand_checked_case():
    """One check over two bits of equal prior 1, syndrome 1, alpha 1, clip 1e6 (pin 2e6), T = 2, Dmax = 2.
    t = 1: b = (1, 1), m1 = 1 at a = 0, m2 = 1, par = 1: c = (-1, -1); L = (1 - 1, 1 - 1) = (0, 0); err = (1, 1): H err = 0,
           not matched.
    t = 2: b = L - c = (1, 1) again: c = (-1, -1), L = (0, 0), not matched.  The round ends, |D| = 0 < 2: both |L| are 0, the
           tie picks bit 0; L[0] = 0 <= 0, so its pin is -2e6.  D = {0}.
    t = 3: the check sweep still reads L = (0, 0): c = (-1, -1).  Bit sweep: L[0] = -2e6 (the pin), L[1] = 1 - 1 = 0;
           err = (1, 1), not matched.
    t = 4: b = (clamp(-2e6 + 1) = -clip, 0 + 1 = 1): mag = (1e6, 1); 1e6 is not < m1 = clip, then m1 = 1 at a = 1 and
           m2 = clip; par = 1 ^ 1 ^ 0 = 0: c = (-1, +clip).  L = (-2000000, 1 + 1000000 = 1000001); err = (1, 0): matched.
    Min-sum alone never gets there: both bits stay tied at posterior 0."""
    H = np.array([[1, 1]], dtype=np.uint8)
    syn = np.array([[1]], dtype=np.uint8)
    # Dmax = 0: the state after t = 2, where the syndrome gives up
    assert [x.tolist() for x in DecimModel(H, [1.0, 1.0], 2, 0, alpha=1.0).decode(syn)] == [[[1, 1]], [0], [2], [0], [[0.0, 0.0]]]
    # T = 1, Dmax = 1: pinned after t = 1, so its t = 2 is the "t = 3" above, and there |D| == Dmax stops it
    err, conv, its, dec, L = DecimModel(H, [1.0, 1.0], 1, 1, alpha=1.0).decode(syn)
    assert L.tolist() == [[-2000000.0, 0.0]] and err.tolist() == [[1, 1]] and conv[0] == 0 and its[0] == 2 and dec[0] == 1
    err, conv, its, dec, L = DecimModel(H, [1.0, 1.0], 2, 2, alpha=1.0).decode(syn)
    assert err.tolist() == [[1, 0]] and conv.tolist() == [1] and its.tolist() == [4] and dec.tolist() == [1]
    assert L.tolist() == [[-2000000.0, 1000001.0]]
    assert (err.dtype, conv.dtype, its.dtype, dec.dtype, L.dtype) == (np.uint8, np.uint8, np.int32, np.int32, np.float32)
    merr, mconv, mits, mL = MinSumModel(H, [1.0, 1.0], 50, alpha=1.0).decode(syn)
    assert mconv[0] == 0 and mits[0] == 50 and mL.tolist() == [[0.0, 0.0]]


@pytest.mark.parametrize("per", [0.03, 0.06])
def test_model_with_no_decimation_is_the_minsum_model(bb72, per):
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 100, per, seed=3))
    prior = llr_of_probs(np.full(72, per))
    err, conv, its, dec, L = DecimModel(bb72, prior, 30, 0).decode(syn)
    merr, mconv, mits, mL = MinSumModel(bb72, prior, 30).decode(syn)
    assert 0 < mconv.sum() < 100 or per == 0.03
    assert np.array_equal(err, merr) and np.array_equal(conv, mconv) and np.array_equal(its, mits) and not dec.any()
    assert np.array_equal(L.view(np.int32), mL.view(np.int32))


def test_model_round_iters_zero_gives_zeros(bb72):
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 5, 0.06, seed=3))
    out = DecimModel(bb72, llr_of_probs(np.full(72, 0.06)), 0, 72).decode(syn)
    assert all(not x.view(np.uint8).any() for x in out) and out[4].shape == (5, 72)


def test_model_column_does_not_depend_on_its_neighbours(bb72):
    """Short rounds, so that one batch holds columns that stop in round 0, columns rescued by a decimation and columns
    that give up."""
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 400, 0.06, seed=3))[:60]
    m = DecimModel(bb72, llr_of_probs(np.full(72, 0.06)), 3, 6)
    err, conv, its, dec, L = full = m.decode(syn)
    assert (conv == 0).any() and ((conv == 1) & (dec == 0)).any() and ((conv == 1) & (dec > 0)).any()
    assert ((conv == 0) <= (dec == 6)).all() and ((conv == 0) <= (its == 21)).all()
    picks = [int(np.nonzero(conv == 0)[0][0]), int(np.nonzero((conv == 1) & (dec == 0))[0][0]), int(np.nonzero((conv == 1) & (dec > 0))[0][-1]), 59]
    for c in picks:
        assert _same(m.decode(syn[c:c + 1]), tuple(x[c:c + 1] for x in full)), c
    perm = np.random.default_rng(1).permutation(60)
    assert _same(m.decode(syn[perm]), tuple(x[perm] for x in full))


def test_bb72_decimation_converges_what_minsum_leaves(bb72):
    """BB-72 H_X, uniform prior, 400 syndromes of errors at 0.06 (seed 3): min-sum(30) converges on 327, decimation with
    rounds of 10 and up to 72 decimations on 398 -- among them every column min-sum converges on -- and every converged
    column reproduces its syndrome with its pinned bits at +-2 clip."""
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    ms = MinSumModel(bb72, prior, 30).decode(syn)
    err, conv, its, dec, L = DecimModel(bb72, prior, 10, 72).decode(syn)
    print(f"min-sum(30): {int(ms[1].sum())} of 400 converged; decimation 10 / 72: {int(conv.sum())}, most decimations {int(dec.max())}, "
          f"most iterations {int(its.max())}")
    assert int(ms[1].sum()) == 327 and int(conv.sum()) == 398
    assert ((ms[1] == 0) | (conv == 1)).all()
    assert np.array_equal(ldpc.codes.syndromes_of(bb72, err[conv == 1]), syn[conv == 1])
    assert np.array_equal((np.abs(L) == np.float32(2e6)).sum(axis=1), dec) and (its <= 10 * (dec + 1)).all()
    assert ((conv == 0) <= (dec == 72)).all()


# ---- the new symbols; ldpc_decim_create validates before it looks for a device ----------------------------------------

def _prototypes(header):
    """name -> (return type, [argument, ...]) of every function the header declares."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"^[ \t]*((?:const\s+)?\w+[\s\*]+)(ldpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        protos[m.group(2)] = (" ".join(m.group(1).split()), [a.strip() for a in m.group(3).split(",")])
    return protos


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_declared_and_bound_as_declared(experiments):
    """The entries are declared in include/ldpc_mi355x_decim.h and the hook in ldpc_mi355x_decim_debug.h, parts of the two
    headers that include them (where the section and the hook are described), and bound from tables of their own: every
    declared function is in its table, exported by both builds, and bound with the types of its declaration."""
    lib = ldpc._capi.lib(experiments)
    main, hook = _prototypes("ldpc_mi355x_decim.h"), _prototypes("ldpc_mi355x_decim_debug.h")
    assert tuple(main) == NEW_SYMBOLS == ldpc._capi.DECIM_SYMBOLS == tuple(ldpc._capi.DECIM_API)
    assert tuple(hook) == ("ldpc_debug_decim_tile_plan",) == ldpc._capi.DECIM_DEBUG_SYMBOLS == tuple(ldpc._capi.DECIM_DEBUG_API)
    assert not set(NEW_SYMBOLS) & set(ldpc._capi.EXPORTED_SYMBOLS) and "ldpc_debug_decim_tile_plan" not in ldpc._capi.DEBUG_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ldpc_mi355x_debug.h")).read()
    assert '#include "ldpc_mi355x_decim.h"' in hdr and "THE RULE" in hdr[hdr.index("Guided-decimation"):hdr.index("ldpc_mi355x_decim.h")]
    assert '#include "ldpc_mi355x_decim_debug.h"' in dbg and "typedef struct ldpc_decim_options" in hdr
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "ldpc_status": ctypes.c_int32}
    for name, (ret, args) in {**main, **hook}.items():
        fn = getattr(lib, name)                                    # (exported by this build)
        assert fn.restype is scalars[ret], (name, ret)
        assert len(fn.argtypes) == len(args), (name, args)
        for got, arg in zip(fn.argtypes, args):
            if "*" in arg:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, arg, got)
            else:
                assert got is scalars[[w for w in arg.split() if w != "const"][0]], (name, arg, got)
    assert lib.ldpc_abi_version() == 4   # added by symbol
    assert ctypes.sizeof(ldpc._capi.DecimOptions) == 64
    assert "DecimatedMinSumDecoder" in ldpc.__all__ and ldpc.DecimatedMinSumDecoder.__mro__[1] is ldpc.AbstractDecoder
    for method in ("decode_batch_host", "decode_batch_device", "decode_", "batchdecode_", "info", "close"):
        assert callable(getattr(ldpc.DecimatedMinSumDecoder, method))


def _create(colptr, rowval, s, n, llr, round_iters=10, max_dec=None, alpha=None, clip=None, variant=0, opts=True, null=()):
    L = ldpc._capi.lib()
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    llr = np.asarray(llr, dtype=np.float32)
    o = ldpc._capi.DecimOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    o.kernel_variant = variant
    h = ctypes.c_void_p()
    st = L.ldpc_decim_create(s, n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                             None if "llr" in null else llr.ctypes.data, round_iters, n if max_dec is None else max_dec,
                             ctypes.byref(o) if opts else None, None if "out" in null else ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_decim_kernel(h) in (1, 2)
        L.ldpc_decim_destroy(h)
    else:
        assert not h.value
    return st, msg


GOOD = dict(colptr=[0, 2, 3, 5], rowval=[0, 1, 1, 0, 2], s=3, n=3, llr=[1.0, -2.0, 3.0])
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.mark.parametrize("change, word", [
    (dict(null=("out",)), "out is NULL"),
    (dict(null=("llr",)), "channel_llr is NULL"),
    (dict(llr=[1.0, np.nan, 3.0]), "channel_llr[1]"),
    (dict(llr=[np.inf, 2.0, 3.0]), "channel_llr[0]"),
    (dict(llr=[1.0, 2.0, -np.inf]), "channel_llr[2]"),
    (dict(round_iters=-1), "round_iters"),
    (dict(max_dec=-1), "max_decimations"),
    (dict(max_dec=4), "max_decimations"),
    (dict(round_iters=2 ** 31 - 1, max_dec=1), "INT32_MAX"),
    (dict(round_iters=2 ** 29, max_dec=3), "INT32_MAX"),
    (dict(round_iters=2 ** 31, max_dec=0), "INT32_MAX"),
    (dict(round_iters=2 ** 62, max_dec=3), "INT32_MAX"),
    (dict(clip=FLT_MAX), "2 * clip"),
    (dict(clip=FLT_MAX * 0.75), "2 * clip"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=-0.25), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(clip=float("inf")), "clip"),
    (dict(clip=-1.0), "clip"),
    (dict(clip=float("nan")), "clip"),
    (dict(variant=3), "kernel_variant"),
    (dict(variant=-1), "kernel_variant"),
    (dict(rowval=[1, 0, 1, 0, 2]), "ascending"),       # unsorted CSC
    (dict(rowval=[0, 1, 1, 0, 3]), "rowval"),          # a row out of range
    (dict(colptr=[0, 2, 3, 4]), "colptr"),
])
def test_create_rejects_bad_arguments_before_any_device_work(change, word):
    st, msg = _create(**{**GOOD, **change})
    assert st == INVALID and word in msg, (st, msg)


def test_create_accepts_the_edges_of_the_ranges_and_a_zeroed_options_struct():
    """Validation passes, and what answers then is the device lookup: LDPC_OK with a GPU, LDPC_ERR_NO_DEVICE without."""
    for kw in (dict(), dict(alpha=0.0, clip=0.0), dict(opts=False), dict(round_iters=0), dict(max_dec=0), dict(max_dec=3),
               dict(round_iters=2 ** 31 - 1, max_dec=0), dict(round_iters=(2 ** 31 - 1) // 4, max_dec=3), dict(clip=FLT_MAX / 2)):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (OK, NO_DEVICE), (st, msg)
        if ldpc._capi.lib().ldpc_device_count() == 0:
            assert st == NO_DEVICE
    L = ldpc._capi.lib()
    assert L.ldpc_decim_kernel(None) == 0 and L.ldpc_decim_tile_syndromes(None) == 0 and L.ldpc_decim_last_grid(None) == 0
    assert L.ldpc_decim_destroy(None) == 0
    assert L.ldpc_decim_decode_batch(None, 1, None, None, None, None, None, None) == INVALID
    assert L.ldpc_decim_decode_batch_device(None, 1, None, None, None, None, None, None, None) == INVALID
    assert "NULL" in L.ldpc_last_error().decode()


# ---- the Python constructor's own refusals ---------------------------------------------------------------------------

H3 = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)


def test_constructor_takes_exactly_one_prior():
    for kw in (dict(per=0.1, channel_probs=[0.1] * 3), dict(per=0.1, channel_llr=[1.0] * 3),
               dict(channel_probs=[0.1] * 3, channel_llr=[1.0] * 3), dict()):
        with pytest.raises(TypeError):
            ldpc.DecimatedMinSumDecoder(H3, kw.pop("per", None), 10, **kw)
    for probs in ([0.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, float("nan")]):
        with pytest.raises(ValueError):
            ldpc.DecimatedMinSumDecoder(H3, None, 10, channel_probs=probs)
    with pytest.raises(ValueError):
        ldpc.DecimatedMinSumDecoder(H3, None, 10, channel_llr=[1.0, 2.0])   # one prior per bit


def test_constructor_checks_types_and_ranges():
    for kw in (dict(max_iters=10.0), dict(max_iters=True), dict(max_decimations=2.0), dict(max_decimations=False), dict(per=1)):
        args = {"per": 0.05, "max_iters": 10, **kw}
        with pytest.raises(TypeError):
            ldpc.DecimatedMinSumDecoder(H3, args.pop("per"), args.pop("max_iters"), **args)
    for kw in (dict(max_iters=-1), dict(max_decimations=-1), dict(max_decimations=4)):
        args = {"max_iters": 10, **kw}
        with pytest.raises(ValueError):
            ldpc.DecimatedMinSumDecoder(H3, 0.05, args.pop("max_iters"), **args)


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")), dict(clip=3e38),
                                dict(max_iters=2 ** 30, max_decimations=2),
                                dict(channel_llr=[1.0, float("nan"), 2.0], per=None), dict(kernel_variant=3)])
def test_constructor_reports_invalid_argument_with_a_message(kw):
    args = {"per": 0.05, "max_iters": 10, **kw}
    with pytest.raises(ldpc.LdpcError) as e:
        ldpc.DecimatedMinSumDecoder(H3, args.pop("per"), args.pop("max_iters"), **args)
    assert e.value.status == INVALID and e.value.message


def test_constructor_hands_over_what_it_documents(monkeypatch):
    """max_decimations=None means n; the defaults are 10 iterations a round; without a device the library answers
    LDPC_ERR_NO_DEVICE after it has accepted the arguments, so they are read off a stub."""
    seen = {}

    class Stub:
        def __getattr__(self, name):
            def call(*a):
                seen[name] = a
                return 0
            return call

    monkeypatch.setattr(ldpc._capi, "lib_for", lambda *_: Stub())
    d = ldpc.DecimatedMinSumDecoder(H3, 0.05, device=0)
    assert (d.max_iters, d.max_decimations, d.alpha, d.clip, d.per) == (10, 3, 0.75, 1e6, 0.05)
    assert np.array_equal(d.channel_llr.view(np.int32), llr_of_probs(np.full(3, 0.05)).view(np.int32))
    a = seen["ldpc_decim_create"]
    assert a[:3] == (2, 3, 4) and a[5] == d.channel_llr.ctypes.data and a[6:8] == (10, 3)
    d = ldpc.DecimatedMinSumDecoder(H3, None, 7, channel_llr=[1.0, 2.0, 3.0], max_decimations=2, device=0)
    assert seen["ldpc_decim_create"][6:8] == (7, 2) and d.per is None and d.scratch.err.shape == (3,)


# ---- the plan --------------------------------------------------------------------------------------------------------------

def state_bytes(s, n, rec_words, S):
    """S lanes of L [n], the records and D [ceil(n / 32)] (words) and the syndrome (bytes), rounded up to 256."""
    return (S * (4 * (n + rec_words + (n + 31) // 32) + s) + 255) // 256 * 256


def plan_of(s, n, rec_words, variant):
    """The policy restated: the widest power of two <= 64 within 79 KiB, else within 159 KiB, else the unlimited tier."""
    S = 0
    for budget in (KIB79, KIB159):
        for w in (64, 32, 16, 8, 4, 2, 1):
            if not S and state_bytes(s, n, rec_words, w) <= budget:
                S = w
    if variant == 1 and not S:
        return UNSUPPORTED
    tier = variant or (1 if S else 2)
    S = S if tier == 1 else 64
    return tier, S, state_bytes(s, n, rec_words, S)


def lib_plan(s, n, rec_words, variant, experiments=False):
    L = ldpc._capi.lib(experiments)
    tier, S, nbytes = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.ldpc_debug_decim_tile_plan(s, n, rec_words, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(nbytes))
    return (tier.value, S.value, nbytes.value) if st == OK else st


@pytest.mark.parametrize("experiments", [False, True])
def test_the_plan_equals_the_formula_over_a_grid_of_sizes(experiments):
    seen = set()
    for n in (0, 1, 2, 31, 32, 33, 72, 150, 240, 600, 1200, 2400, 4800, 9600, 13000, 16384, 40000):
        for s in sorted({0, 1, n // 2, n}):
            for rec in sorted({0, 4 * s, 5 * s + 70}):
                for variant in (0, 1, 2):
                    want = plan_of(s, n, rec, variant)
                    assert lib_plan(s, n, rec, variant, experiments) == want, (s, n, rec, variant)
                    seen.add(want if want == UNSUPPORTED else want[:2])
    assert {(1, w) for w in (64, 32, 16, 8, 4, 2, 1)} | {(2, 64), UNSUPPORTED} <= seen


def test_the_plans_of_the_shapes_the_gpu_tests_use():
    assert lib_plan(36, 72, 144, 0) == (1, 64, 58368) and 4 * (72 + 144 + 3) + 36 == 912               # BB-72
    assert lib_plan(36, 72, 144, 2) == (2, 64, 58368)
    assert 4 * (240 + 480 + 8) + 120 == 3032 and lib_plan(120, 240, 480, 0) == (1, 16, 16 * 3032 + 128)  # (240, 8, 4): 48512 -> 48640
    assert lib_plan(1, 2, 4, 0) == (1, 64, state_bytes(1, 2, 4, 64))                                     # the hand case: one partial D word
    # one syndrome of (16384, 8, 4) takes 206848 bytes > 159 KiB
    assert 4 * (16384 + 32768 + 512) + 8192 == 206848 > KIB159
    assert lib_plan(8192, 16384, 32768, 0) == (2, 64, 64 * 206848) and lib_plan(8192, 16384, 32768, 1) == UNSUPPORTED
    assert "on-chip" in ldpc._capi.lib().ldpc_last_error().decode()
    for bad in ((-1, 72, 144, 0), (36, -1, 144, 0), (36, 72, -1, 0), (36, 72, 144, 3), (36, 72, 144, -1), (1 << 28, 72, 144, 0),
                (36, 1 << 28, 144, 0), (36, 72, 1 << 31, 0)):
        assert lib_plan(*bad) == INVALID, bad
    assert ldpc._capi.lib().ldpc_debug_decim_tile_plan(36, 72, 144, 0, None, None, None) == OK   # every out may be NULL


# ---- the planner addition under the sanitizers ------------------------------------------------------------------------------

def test_decim_plan_under_sanitizers(tmp_path):
    """csrc/tile_plan.hpp (decim_tile_plan and decim_state_bytes) built with AddressSanitizer + UBSan (CPU only) and driven
    by tests/native/decim_plan_sanitize.cpp: a program of its own, nothing is preloaded."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "decim_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "decim_plan_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK ") and "decimation plans" in out.stdout, out.stdout + out.stderr


# ---- the table of tests/test_gpu_decim_widths.py ------------------------------------------------------------------------------
# (3,6)-regular graphs of parity_check_csc(n, 6, 3): s = n / 2, rec_words = 2 n, so a lane takes
# 4 (n + 2 n + ceil(n / 32)) + n / 2 = 12.625 n bytes (n a multiple of 32).  n -> (tier, S, the budget S was found under)
DECIM_TABLE = {
    96: (1, 64, KIB79),
    192: (1, 32, KIB79),
    384: (1, 16, KIB79),
    768: (1, 8, KIB79),
    1536: (1, 4, KIB79),
    3072: (1, 2, KIB79),
    6144: (1, 1, KIB79),
    6432: (1, 2, KIB159),     # 81204 bytes a lane miss 79 KiB; two lanes, 162408 -> 162560, fit 159 KiB: S = 2, not 1
    12288: (1, 1, KIB159),    # 155136 bytes: one workgroup a CU
    13824: (2, 64, 0),        # 174528 bytes a lane: the unlimited tier by size
}


@pytest.mark.parametrize("experiments", [False, True])
@pytest.mark.parametrize("n", sorted(DECIM_TABLE))
def test_the_table_of_the_width_tests(n, experiments):
    tier, S, budget = DECIM_TABLE[n]
    s, rec = n // 2, 2 * n
    assert n % 32 == 0 and 4 * (n + rec + n // 32) + s == 12.625 * n                # the per-lane formula ...
    assert state_bytes(s, n, rec, 1) == -(-int(12.625 * n) // 256) * 256             # ... and the 256-byte rounding of a tile
    assert plan_of(s, n, rec, 0) == (tier, S, state_bytes(s, n, rec, S))           # the row follows from the restated rule
    assert lib_plan(s, n, rec, 0, experiments) == (tier, S, state_bytes(s, n, rec, S))
    if tier == 1:
        assert lib_plan(s, n, rec, 1, experiments) == (tier, S, state_bytes(s, n, rec, S))
        assert state_bytes(s, n, rec, S) <= budget and (S == 64 or state_bytes(s, n, rec, 2 * S) > budget)
        assert (budget == KIB79) == (state_bytes(s, n, rec, 1) <= KIB79)          # 159 KiB is tried only where 79 KiB holds nothing
    else:
        assert state_bytes(s, n, rec, 1) > KIB159 and lib_plan(s, n, rec, 1, experiments) == UNSUPPORTED
        assert "on-chip" in ldpc._capi.lib(experiments).ldpc_last_error().decode()
    assert lib_plan(s, n, rec, 2, experiments) == (2, 64, state_bytes(s, n, rec, 64))
    if n == 6432:      # the window: one lane lies in (79 KiB, 159 KiB / 2]
        assert (int(12.625 * n), state_bytes(s, n, rec, 2)) == (81204, 162560) and KIB79 < 81204 <= KIB159 // 2
    if n == 12288:
        assert state_bytes(s, n, rec, 1) == 155136
    if n == 13824:
        assert int(12.625 * n) == 174528


# ---- the model's additions for the tests of the tie rule ----------------------------------------------------------------------

def test_model_tie_argument_and_tie_count(bb72):
    """The hand case: at its one decimation both |L| are 0, a tie; "highest" pins bit 1 where the rule pins bit 0, with the
    mirrored outcome.  On BB-72 with the uniform prior ties occur and change LLRs; with distinct priors on a graph without
    symmetry no tie occurs and the two coincide.  The default is the rule, and `last_ties` is reset by every decode."""
    H = np.array([[1, 1]], dtype=np.uint8)
    syn = np.array([[1]], dtype=np.uint8)
    low, high = DecimModel(H, [1.0, 1.0], 2, 2, alpha=1.0), DecimModel(H, [1.0, 1.0], 2, 2, alpha=1.0, tie="highest")
    assert _same(low.decode(syn), DecimModel(H, [1.0, 1.0], 2, 2, alpha=1.0, tie="lowest").decode(syn))
    assert high.decode(syn)[4].tolist() == [[1000001.0, -2000000.0]] and low.decode(syn)[4].tolist() == [[-2000000.0, 1000001.0]]
    assert (low.last_ties, high.last_ties) == (1, 1)
    assert low.decode(np.array([[0]], dtype=np.uint8))[1][0] == 1 and low.last_ties == 0          # reset; no decimation, no tie
    with pytest.raises(AssertionError):
        DecimModel(H, [1.0, 1.0], 2, 2, tie="first")
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 60, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    low, high = DecimModel(bb72, prior, 3, 6), DecimModel(bb72, prior, 3, 6, tie="highest")
    a, b = low.decode(syn), high.decode(syn)
    assert 0 < low.last_ties <= int(a[3].sum()) and (a[4].view(np.int32) != b[4].view(np.int32)).any()
    assert _same(DecimModel(bb72, prior, 0, 6, tie="highest").decode(syn), DecimModel(bb72, prior, 0, 6).decode(syn))
    rng = np.random.default_rng(2)
    distinct = llr_of_probs(rng.uniform(0.01, 0.2, 72))
    low, high = DecimModel(bb72, distinct, 3, 6), DecimModel(bb72, distinct, 3, 6, tie="highest")
    a, b = low.decode(syn), high.decode(syn)
    assert a[3].sum() > 0 and (low.last_ties > 0 or _same(a, b))                       # no tie: the two rules are one
