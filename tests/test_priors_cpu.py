"""Min-sum with per-syndrome priors without a GPU: the numpy models of tests/priors_model.py against the models they were
made from, the second tile plan (ldpc_debug_priors_tile_plan) against the rule restated here, the new symbols and their
refusals before any device work, `conditional_probs`, the effect of conditioning the second decode of a CSS code on the
first (on the models alone), and the planner addition under the sanitizers."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import ldpcdecoders_jl_amd as ldpc
import priors_model as pm
from layered_model import LayeredMinSumModel
from minsum_model import MinSumModel, llr_of_probs

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5
KIB79, KIB159 = 79 * 1024, 159 * 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldpc_minsum_decode_batch_priors_device", "ldpc_minsum_decode_batch_priors", "ldpc_minsum_set_conditional_priors",
               "ldpc_minsum_decode_batch_given_device", "ldpc_minsum_decode_batch_given", "ldpc_minsum_priors_kernel",
               "ldpc_minsum_priors_tile_syndromes")


def _bb72():
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx, dtype=np.uint8)), sp.csc_matrix(np.asarray(Hz, dtype=np.uint8))


def _same_bits(got, want, what):
    for g, w, name in zip(got, want, ("err", "conv", "iters", "L")):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {name} differs"


# ---- the models ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_equal_rows_give_the_model_with_a_shared_prior(schedule):
    H, _ = _bb72()
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 64, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    shared = (LayeredMinSumModel if schedule == "layered" else MinSumModel)(H, prior, 30).decode(syn)
    assert 0 < shared[1].sum() < 64
    _same_bits(pm.model_of(schedule, H, 30).decode(syn, np.tile(prior, (64, 1))), shared, schedule)
    # per-bit priors, and max_iters = 0
    prior = llr_of_probs(np.random.default_rng(1).uniform(0.01, 0.3, 72))
    shared = (LayeredMinSumModel if schedule == "layered" else MinSumModel)(H, prior, 7, alpha=1.0, clip=8.0).decode(syn)
    _same_bits(pm.model_of(schedule, H, 7, 1.0, 8.0).decode(syn, np.tile(prior, (64, 1))), shared, schedule + ", per bit")
    out = pm.model_of(schedule, H, 0).decode(syn, np.tile(prior, (64, 1)))
    assert not any(x.view(np.uint8).any() for x in out)


@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_a_row_depends_on_its_own_priors_only_and_a_non_finite_row_is_not_decoded(schedule):
    H, _ = _bb72()
    rng = np.random.default_rng(4)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 12, 0.06, seed=8))
    a, b = llr_of_probs(rng.uniform(0.02, 0.4, 72)), llr_of_probs(rng.uniform(0.02, 0.4, 72))
    given = rng.integers(0, 4, size=(12, 72), dtype=np.uint8)
    pri = pm.select_priors(given, a, b)
    assert np.array_equal(pri, np.where((given & 1) == 1, b, a)) and (given > 1).any()
    model = pm.model_of(schedule, H, 20)
    whole = model.decode(syn, pri)
    for c in (0, 5, 11):   # row c alone, under the model with that row's prior as the shared one
        alone = (LayeredMinSumModel if schedule == "layered" else MinSumModel)(H, pri[c], 20).decode(syn[c:c + 1])
        _same_bits(tuple(x[c:c + 1] for x in whole), alone, f"{schedule} row {c}")
    bad = pri.copy()
    bad[2, 7], bad[9, 71] = np.nan, -np.inf
    out = model.decode(syn, bad)
    for c in (2, 9):
        assert not out[0][c].any() and out[1][c] == 0 and out[2][c] == 0 and not out[3][c].view(np.int32).any()
    keep = [c for c in range(12) if c not in (2, 9)]
    _same_bits(tuple(x[keep] for x in out), tuple(x[keep] for x in whole), schedule + " the other rows")


# ---- the second plan ----------------------------------------------------------------------------------------------------

def plain_bytes(s, n, rec_words, S):
    return ((4 * (n + rec_words) + s) * S + 255) // 256 * 256


def priors_bytes(s, n, rec_words, S):
    """the plain blocks, the next word boundary, then P [n][S] f32; rounded up to 256"""
    return (((4 * (n + rec_words) + s) * S + 3) // 4 * 4 + 4 * n * S + 255) // 256 * 256


def rule(size_of, variant=0):
    S = 0
    for budget in (KIB79, KIB159):
        fits = [w for w in (64, 32, 16, 8, 4, 2, 1) if size_of(w) <= budget]
        if fits:
            S = fits[0]
            break
    if variant == 1:
        return (1, S, size_of(S)) if S else None
    if variant == 2:
        return (2, 64, size_of(64))
    return (1, S, size_of(S)) if S else (2, 64, size_of(64))


def lib_plan(name, s, n, rec_words, flag, variant, experiments=False):
    L = ldpc._capi.lib(experiments)
    tier, S, nbytes = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int64(-7)
    st = getattr(L, name)(s, n, rec_words, flag, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(nbytes))
    return (tier.value, S.value, nbytes.value) if st == OK else st


@pytest.mark.parametrize("experiments", [False, True])
def test_the_priors_plan_of_regular_8_4_graphs(experiments):
    """s = n / 2, four-word records: rec_words = 2 n; 12.5 n bytes a syndrome plain, 16.5 n with the priors block."""
    for n in (96, 10240, 72, 240, 1024, 2048, 4096):
        s, rec = n // 2, 2 * n
        assert 4 * (n + rec) + s == 12.5 * n and priors_bytes(s, n, rec, 1) == (int(16.5 * n) + 255) // 256 * 256 and 16.5 * n == int(16.5 * n)
        for variant in (0, 1, 2):
            want_plain = rule(lambda S: plain_bytes(s, n, rec, S), variant)
            want_priors = rule(lambda S: priors_bytes(s, n, rec, S), variant)
            assert lib_plan("ldpc_debug_tile_plan", s, n, rec, 0, variant, experiments) == (want_plain or UNSUPPORTED)
            assert lib_plan("ldpc_debug_priors_tile_plan", s, n, rec, 0, variant, experiments) == (want_priors or UNSUPPORTED), (n, variant)
            # a layered handle keeps no priors block: its priors plan is its plain plan
            assert lib_plan("ldpc_debug_priors_tile_plan", s, n, rec, 1, variant, experiments) == (want_plain or UNSUPPORTED)
    # the two shapes of the proposal, spelled out
    assert rule(lambda S: plain_bytes(48, 96, 192, S))[:2] == (1, 64) and rule(lambda S: priors_bytes(48, 96, 192, S))[:2] == (1, 32)
    assert lib_plan("ldpc_debug_priors_tile_plan", 48, 96, 192, 0, 0, experiments)[:2] == (1, 32)
    assert rule(lambda S: plain_bytes(5120, 10240, 20480, S))[:2] == (1, 1) and rule(lambda S: priors_bytes(5120, 10240, 20480, S))[:2] == (2, 64)
    assert lib_plan("ldpc_debug_tile_plan", 5120, 10240, 20480, 0, 0, experiments)[:2] == (1, 1)
    assert lib_plan("ldpc_debug_priors_tile_plan", 5120, 10240, 20480, 0, 0, experiments)[:2] == (2, 64)
    assert rule(lambda S: priors_bytes(5120, 10240, 20480, S), 1) is None
    assert lib_plan("ldpc_debug_priors_tile_plan", 5120, 10240, 20480, 0, 1, experiments) == UNSUPPORTED
    assert lib_plan("ldpc_debug_tile_plan", 5120, 10240, 20480, 0, 1, experiments)[:2] == (1, 1)


def test_bb72_stays_at_64_syndromes_and_odd_sizes_keep_the_block_on_a_word():
    H, _ = _bb72()
    deg = np.diff(sp.csr_matrix(H).indptr)
    rec = int(4 * len(deg))
    assert set(deg) == {6}
    assert lib_plan("ldpc_debug_tile_plan", 36, 72, rec, 0, 0)[:2] == (1, 64)
    assert lib_plan("ldpc_debug_priors_tile_plan", 36, 72, rec, 0, 0) == (1, 64, priors_bytes(36, 72, rec, 64))
    # s S not a multiple of four: the block moves to the next word
    for s, n, rec in ((3, 5, 8), (1, 1, 4), (7, 40000, 28), (13, 20000, 52)):
        want = rule(lambda S: priors_bytes(s, n, rec, S))
        assert lib_plan("ldpc_debug_priors_tile_plan", s, n, rec, 0, 0) == want, (s, n, rec)
    assert priors_bytes(7, 40000, 28, 1) > plain_bytes(7, 40000, 28, 1) + 160000 - 256
    for bad in ((-1, 4, 0, 0, 0), (4, -1, 0, 0, 0), (4, 4, -1, 0, 0), (4, 4, 0, 2, 0), (4, 4, 0, -1, 0), (4, 4, 0, 0, 3), (1 << 28, 4, 0, 0, 0)):
        assert lib_plan("ldpc_debug_priors_tile_plan", *bad) == INVALID, bad
    assert ldpc._capi.lib().ldpc_debug_priors_tile_plan(36, 72, 144, 0, 0, None, None, None) == OK   # every out may be NULL


# ---- symbols and refusals -------------------------------------------------------------------------------------------------

def _prototypes(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(2): (m.group(1), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b(ldpc_status|int32_t)\s+(ldpc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def _ctype_of(arg):
    if "*" in arg:
        return "pointer"
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[arg.split()[0]]


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_listed_and_declared_as_in_the_header(experiments):
    L = ldpc._capi.lib(experiments)
    assert L.ldpc_abi_version() == 4
    protos = {**_prototypes("ldpc_mi355x.h"), **_prototypes("ldpc_mi355x_debug.h")}
    for name in NEW_SYMBOLS + ("ldpc_debug_priors_tile_plan",):
        assert name in (ldpc._capi.DEBUG_SYMBOLS if "debug" in name else ldpc._capi.EXPORTED_SYMBOLS), name
        assert (name in _prototypes("ldpc_mi355x_debug.h")) == ("debug" in name)
        fn = getattr(L, name)
        ret, args = protos[name]
        assert fn.restype is ctypes.c_int32                                # ldpc_status is an int; the getters are int32_t
        assert len(fn.argtypes) == len(args), (name, args)
        for got, arg in zip(fn.argtypes, args):
            want = _ctype_of(arg)
            if want == "pointer":
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, arg, got)
            else:
                assert got is want, (name, arg, got)
    assert len(protos["ldpc_minsum_decode_batch_priors_device"][1]) == 9 and len(protos["ldpc_minsum_decode_batch_given"][1]) == 8
    assert L.ldpc_minsum_priors_kernel(None) == 0 and L.ldpc_minsum_priors_tile_syndromes(None) == 0


def test_refusals_before_any_device_work():
    """Without a handle nothing can reach a device: a NULL handle is refused by every new entry, with a message.  (The
    refusals that need a handle -- NULL pointers, tables not set, non-finite tables -- are in tests/test_gpu_priors.py.)"""
    L = ldpc._capi.lib()
    buf = np.zeros(8, dtype=np.float32)
    calls = [
        lambda: L.ldpc_minsum_decode_batch_priors_device(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None),
        lambda: L.ldpc_minsum_decode_batch_priors(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None),
        lambda: L.ldpc_minsum_decode_batch_given_device(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None),
        lambda: L.ldpc_minsum_decode_batch_given(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None),
        lambda: L.ldpc_minsum_decode_batch_priors(None, 0, None, None, None, None, None, None),
        lambda: L.ldpc_minsum_decode_batch_given_device(None, -1, None, None, None, None, None, None, None),
        lambda: L.ldpc_minsum_set_conditional_priors(None, buf.ctypes.data, buf.ctypes.data),
    ]
    for k, call in enumerate(calls):
        assert call() == INVALID, k
        assert "NULL" in L.ldpc_last_error().decode(), k


def test_python_methods_exist_and_the_trials_loop_refuses_another_decoder_hx():
    for name in ("decode_batch_priors_host", "decode_batch_priors_device", "set_conditional_priors", "decode_batch_given_host",
                 "decode_batch_given_device"):
        assert callable(getattr(ldpc.MinSumDecoder, name))
    import inspect

    sig = inspect.signature(ldpc.run_css_trials)
    assert sig.parameters["correlated"].default is False and list(sig.parameters)[-1] == "correlated"

    class NotMinSum:
        pass
    with pytest.raises(TypeError, match="MinSumDecoder"):
        ldpc.run_css_trials(NotMinSum(), NotMinSum(), 10, 0.06, correlated=True)
    osd = object.__new__(ldpc.BeliefPropagationOSDDecoder)             # a BP+OSD wrapper is not a min-sum decoder either
    with pytest.raises(TypeError, match="MinSumDecoder"):
        ldpc.run_css_trials(osd, NotMinSum(), 10, 0.06, correlated=True)


# ---- conditional_probs ----------------------------------------------------------------------------------------------------

def test_conditional_probs():
    for p in (0.06, 0.045, 0.001, 0.3):
        for fn in (ldpc.conditional_probs, ldpc.css_trials.conditional_probs, pm.conditional_probs):
            p0, p1 = fn(p)
            assert p1 == 0.5 and p0 == pytest.approx((p / 3) / (1 - 2 * p / 3), rel=1e-15) and isinstance(p0, float)
        assert ldpc.conditional_probs(p) == pm.conditional_probs(p)
    # biased noise: a triple is taken as it is
    assert ldpc.conditional_probs((0.01, 0.03, 0.02)) == (0.02 / (1 - 0.01 - 0.03), 0.03 / (0.01 + 0.03)) == pm.conditional_probs((0.01, 0.03, 0.02))
    for bad in ((0.0, 0.0, 0.05), (0.02, 0.0, 0.01), (0.0, 0.02, 0.01), (0.01, 0.01, 0.0), (0.25, 0.25, 0.5), 0.0):
        with pytest.raises(ValueError):
            ldpc.conditional_probs(bad)
    for bad in ((0.0, 0.0, 0.05), 0.0):
        with pytest.raises(ValueError):
            pm.conditional_probs(bad)


# ---- the effect, on the models alone ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _effect_inputs():
    Hx, Hz = _bb72()
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    ex, ez = cm.sample(72, 400, 0.06, seed=0)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    return Hx, Hz, Lx, Lz, ex, ez, sx, sz


@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_conditioning_the_second_decode_lowers_the_logical_z_failures(schedule):
    """BB-72, depolarizing 0.06, 400 trials of sampler seed 0, 30 iterations, alpha 0.75.  Independent: both sides with the
    marginal 2 p / 3.  Conditioned: the decode on Hx takes, per trial and qubit, the prior chosen by the guess gx of the
    decode on Hz.  Measured when this was written: flooding 52 -> 24, layered 47 -> 18 logical-Z failures."""
    Hx, Hz, Lx, Lz, ex, ez, sx, sz = _effect_inputs()
    marginal = llr_of_probs(np.full(72, 2 * 0.06 / 3))
    Shared = LayeredMinSumModel if schedule == "layered" else MinSumModel
    gx = Shared(Hz, marginal, 30).decode(sz)[0]
    gz_independent = Shared(Hx, marginal, 30).decode(sx)[0]
    p_if0, p_if1 = pm.conditional_probs(0.06)
    pri = pm.select_priors(gx, llr_of_probs(np.full(72, p_if0)), llr_of_probs(np.full(72, p_if1)))
    gz_conditioned = pm.model_of(schedule, Hx, 30).decode(sx, pri)[0]
    _, before = cm.score(Hx, Hz, Lx, Lz, gx, gz_independent, ex, ez)
    _, after = cm.score(Hx, Hz, Lx, Lz, gx, gz_conditioned, ex, ez)
    print(f"{schedule}: logical-Z failures {int(before[5])} -> {int(after[5])}, logical-X {int(before[4])} -> {int(after[4])}, "
          f"any {int(before[3])} -> {int(after[3])} of 400")
    assert after[5] < before[5]
    assert after[4] == before[4]


# ---- the planner addition under the sanitizers ------------------------------------------------------------------------------

def test_priors_plan_under_sanitizers(tmp_path):
    """csrc/tile_plan.hpp (priors_tile_plan and the two size functions) built with AddressSanitizer + UBSan (CPU only) and
    driven by tests/native/priors_plan_sanitize.cpp."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "priors_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "priors_plan_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK ") and "priors plans" in out.stdout, out.stdout + out.stderr
