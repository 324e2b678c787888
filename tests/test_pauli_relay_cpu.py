"""Pauli relay min-sum decoder without a GPU: the planner sizes (csrc/tile_plan.hpp pauli_relay_tile_plan through
ldpc_debug_pauli_relay_tile_plan) at hand-computed shapes and under the sanitizers, the new symbols, the argument
validation of ldpc_pauli_relay_create (which answers before any device work), the Python constructor's own refusals, and the
numpy model of the rule (tests/pauli_relay_model.py): the consequence that ties it to the Pauli min-sum model, a
hand-checked case, the statistical comparison the decoder was built for, and a stopped column that stays frozen."""
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
from pauli_model import PauliMinSumModel, depolarizing_priors
from pauli_relay_model import PauliRelayModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5
KIB79, KIB159 = 79 * 1024, 159 * 1024
NEW_SYMBOLS = ("ldpc_pauli_relay_create", "ldpc_pauli_relay_destroy", "ldpc_pauli_relay_kernel", "ldpc_pauli_relay_tile_syndromes",
               "ldpc_pauli_relay_last_grid", "ldpc_pauli_relay_decode_batch", "ldpc_pauli_relay_decode_batch_device")


# ---- the planner --------------------------------------------------------------------------------------------------------

def lib_plan(s, n, rec_words, variant=0, experiments=False):
    """(tier, S, state bytes) of the library's plan, or its status where it refuses."""
    L = ldpc._capi.lib(experiments)
    tier, S, state = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.ldpc_debug_pauli_relay_tile_plan(s, n, rec_words, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(state))
    return (tier.value, S.value, state.value) if st == OK else st


def lane_bytes(s, n, rec_words):
    """One syndrome: G and M (3 n words each), the records, two bit planes of best (words), the syndrome (bytes)."""
    return 4 * (6 * n + rec_words + 2 * ((n + 31) // 32)) + s


def state_bytes(s, n, rec_words, S):
    return (S * lane_bytes(s, n, rec_words) + 255) // 256 * 256


@pytest.mark.parametrize("s, n, rec_words, variant, want", [
    # BB-72: 36 + 36 checks of degree 6 -> 288 record words; 4 (432 + 288 + 6) + 72 = 2976 B a syndrome; 32 of them are
    # 95232 B > 79 KiB = 80896 B, 16 of them 47616 B
    (72, 72, 288, 0, (1, 16, 47616)),
    (72, 72, 288, 1, (1, 16, 47616)),
    (72, 72, 288, 2, (2, 64, 190464)),
    # the hypergraph product of two 3-bit repetition checks: n = 13, 48 words; 4 (78 + 48 + 2) + 12 = 524 B a syndrome
    (12, 13, 48, 0, (1, 64, 33536)),
    # 4 (1350 + 864 + 16) + 216 = 9136 B a syndrome: 16 of them 146176 B > 80896 B, 8 of them 73088 B -> 73216
    (216, 225, 864, 0, (1, 8, 73216)),
    # 4 (24000 + 16000 + 250) + 4000 = 165000 B a syndrome: past 159 KiB = 162816 B
    (4000, 4000, 16000, 0, (2, 64, 10560000)),
    (4000, 4000, 16000, 2, (2, 64, 10560000)),
    # an empty graph still has its syndrome bytes: 64 * 3 = 192 B -> 256
    (3, 0, 0, 0, (1, 64, 256)),
])
def test_planner_sizes_at_hand_computed_shapes(s, n, rec_words, variant, want):
    assert lib_plan(s, n, rec_words, variant) == want
    assert want[2] == state_bytes(s, n, rec_words, want[1])


def test_planner_refusals():
    assert 4 * (24000 + 16000 + 250) + 4000 == 165000 > KIB159
    assert lib_plan(4000, 4000, 16000, 1) == UNSUPPORTED          # forced on-chip, nothing fits
    assert "on-chip" in ldpc._capi.lib().ldpc_last_error().decode()
    for bad in ((72, 72, 288, 3), (72, 72, 288, -1), (-1, 72, 288, 0), (72, -1, 288, 0), (72, 72, -1, 0), (72, 1 << 28, 0, 0),
                (1 << 28, 72, 288, 0), (72, 72, 1 << 31, 0)):
        assert lib_plan(*bad) == INVALID, bad
    assert ldpc._capi.lib().ldpc_debug_pauli_relay_tile_plan(72, 72, 288, 0, None, None, None) == OK   # every out may be NULL


def test_pauli_relay_plan_under_sanitizers(tmp_path):
    """csrc/tile_plan.hpp (pauli_relay_tile_plan and pauli_relay_state_bytes) built with AddressSanitizer + UBSan (CPU only)
    and driven by tests/native/pauli_relay_plan_sanitize.cpp: a program of its own, nothing is preloaded."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "pauli_relay_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "pauli_relay_plan_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK ") and "Pauli relay plans" in out.stdout, out.stdout + out.stderr


# ---- the table of tests/test_gpu_pauli_relay_widths.py ----------------------------------------------------------------------
# The core is the hypergraph product of two 3-bit repetition checks (n = 13, 6 + 6 checks, 48 record words), padded with
# isolated qubits up to n and with `empty` empty checks (half behind each side), so a lane takes
# 4 (6 n + 48 + 2 ceil(n / 32)) + 12 + empty bytes.  n -> (empty, tier, S, the budget S was found under)
WIDTH_TABLE = {
    32: (4, 1, 64, KIB79),        # 984 B a lane
    64: (4, 1, 32, KIB79),        # 1760 B
    160: (4, 1, 16, KIB79),       # 4088 B
    320: (4, 1, 8, KIB79),        # 7968 B
    640: (4, 1, 4, KIB79),        # 15728 B
    1280: (4, 1, 2, KIB79),       # 31248 B
    2560: (4, 1, 1, KIB79),       # 62288 B
    3328: (4, 1, 2, KIB159),      # 80912 B a lane miss 79 KiB by 16; two lanes, 161824 -> 162048, fit 159 KiB: S = 2, not 1
    6705: (12, 1, 1, KIB159),     # 162816 B = 159 KiB exactly: the largest state that launches on chip
    6784: (4, 2, 64, 0),          # 164720 B a lane: the unlimited tier by size
}
WIDTH_LANE_BYTES = {32: 984, 64: 1760, 160: 4088, 320: 7968, 640: 15728, 1280: 31248, 2560: 62288, 3328: 80912, 6705: 162816,
                    6784: 164720}


@pytest.mark.parametrize("experiments", [False, True])
@pytest.mark.parametrize("n", sorted(WIDTH_TABLE))
def test_the_table_of_the_width_tests(n, experiments):
    empty, tier, S, budget = WIDTH_TABLE[n]
    s, rec = 12 + empty, 48
    assert lane_bytes(s, n, rec) == WIDTH_LANE_BYTES[n] == 24 * n + 8 * ((n + 31) // 32) + 204 + empty
    assert lib_plan(s, n, rec, 0, experiments) == (tier, S, state_bytes(s, n, rec, S))
    if tier == 1:
        assert lib_plan(s, n, rec, 1, experiments) == (tier, S, state_bytes(s, n, rec, S))
        assert state_bytes(s, n, rec, S) <= budget and (S == 64 or state_bytes(s, n, rec, 2 * S) > budget)
        assert (budget == KIB79) == (state_bytes(s, n, rec, 1) <= KIB79)          # 159 KiB is tried only where 79 KiB holds nothing
    else:
        assert state_bytes(s, n, rec, 1) > KIB159 and lib_plan(s, n, rec, 1, experiments) == UNSUPPORTED
    assert lib_plan(s, n, rec, 2, experiments) == (2, 64, state_bytes(s, n, rec, 64))
    if n == 3328:      # the window: one lane lies in (79 KiB, 159 KiB / 2]
        assert KIB79 < 80912 <= KIB159 // 2 and state_bytes(s, n, rec, 2) == 162048
    if n == 6705:      # one more empty check and nothing fits
        assert state_bytes(s, n, rec, 1) == KIB159 == 162816 and lib_plan(s + 1, n, rec, 0, experiments)[:2] == (2, 64)
        assert lib_plan(s + 1, n, rec, 1, experiments) == UNSUPPORTED


# ---- symbols ------------------------------------------------------------------------------------------------------------

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
    """The entries are declared in include/ldpc_mi355x_pauli_relay.h and the hook in ldpc_mi355x_pauli_relay_debug.h, parts
    of the two headers that include them (where the rule and the hook are described), and bound from tables of their own:
    every declared function is in its table, exported by both builds, and bound with the types of its declaration."""
    lib = ldpc._capi.lib(experiments)
    main, hook = _prototypes("ldpc_mi355x_pauli_relay.h"), _prototypes("ldpc_mi355x_pauli_relay_debug.h")
    assert tuple(main) == NEW_SYMBOLS == ldpc._capi.PAULI_RELAY_SYMBOLS == tuple(ldpc._capi.PAULI_RELAY_API)
    assert tuple(hook) == ("ldpc_debug_pauli_relay_tile_plan",) == ldpc._capi.PAULI_RELAY_DEBUG_SYMBOLS == tuple(ldpc._capi.PAULI_RELAY_DEBUG_API)
    assert not set(NEW_SYMBOLS) & set(ldpc._capi.EXPORTED_SYMBOLS) and "ldpc_debug_pauli_relay_tile_plan" not in ldpc._capi.DEBUG_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    dbg = open(os.path.join(ROOT, "include", "ldpc_mi355x_debug.h")).read()
    assert '#include "ldpc_mi355x_pauli_relay.h"' in hdr and "THE RULE" in hdr[hdr.index("Pauli relay min-sum decoder"):hdr.index("ldpc_mi355x_pauli_relay.h")]
    assert '#include "ldpc_mi355x_pauli_relay_debug.h"' in dbg and "typedef struct ldpc_pauli_relay_options" in hdr
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
    assert ctypes.sizeof(ldpc._capi.PauliRelayOptions) == 64
    assert "PauliRelayMinSumDecoder" in ldpc.__all__ and ldpc.PauliRelayMinSumDecoder is ldpc.pauli_relay.PauliRelayMinSumDecoder
    for member in ("decode_batch_host", "decode_batch_device", "info", "close", "kernel", "tile_syndromes", "last_grid"):
        assert hasattr(ldpc.PauliRelayMinSumDecoder, member)


# ---- ldpc_pauli_relay_create validates before it looks for a device ---------------------------------------------------------

def _pattern(rows, colptr, rowval, keep):
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    keep += [colptr, rowval]
    pat = ldpc._capi.CSSPattern()
    pat.rows, pat.nnz, pat.colptr, pat.rowval = rows, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data
    return pat


# n = 4: Hx = [1 1 1 1], Hz = [1 1 0 0; 0 0 1 1]; two legs
GOOD = dict(n=4, hx=(1, [0, 1, 2, 3, 4], [0, 0, 0, 0]), hz=(2, [0, 1, 2, 3, 4], [0, 0, 1, 1]),
            px=[3.0, 3.0, 3.0, 3.0], py=[3.5, 3.0, 3.0, -1.0], pz=[3.0, 2.0, 3.0, 3.0],
            gammas=[[0.125] * 4, [-0.2, 0.0, 0.5, 0.9]], leg_iters=[5, 3])


def _create(n, hx, hz, px, py, pz, gammas, leg_iters, legs=None, stop_after=None, alpha=None, clip=None, variant=0, opts=True, out=True):
    L = ldpc._capi.lib()
    keep = []
    pats = [ctypes.byref(_pattern(*h, keep)) if h is not None else None for h in (hx, hz)]
    tables = [np.asarray(t, dtype=np.float32) if t is not None else None for t in (px, py, pz)]
    g = np.ascontiguousarray(gammas, dtype=np.float32) if gammas is not None else None
    li = np.ascontiguousarray(leg_iters, dtype=np.int32) if leg_iters is not None else None
    o = ldpc._capi.PauliRelayOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    if stop_after is not None:
        o.stop_after = stop_after
    o.kernel_variant = variant
    h = ctypes.c_void_p()
    st = L.ldpc_pauli_relay_create(n, pats[0], pats[1], *(t.ctypes.data if t is not None else None for t in tables),
                                   (len(li) if li is not None else 1) if legs is None else legs, g.ctypes.data if g is not None else None,
                                   li.ctypes.data if li is not None else None, ctypes.byref(o) if opts else None,
                                   ctypes.byref(h) if out else None)
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_pauli_relay_kernel(h) in (1, 2) and L.ldpc_pauli_relay_last_grid(h) == 0
        L.ldpc_pauli_relay_destroy(h)
    else:
        assert not h.value
    return st, msg


@pytest.mark.parametrize("change, word", [
    (dict(out=False), "out is NULL"),
    (dict(px=None), "prior_x"),
    (dict(py=None), "prior_y"),
    (dict(pz=None), "prior_z"),
    (dict(px=[1.0, np.nan, 3.0, 3.0]), "prior_x[1]"),
    (dict(py=[np.inf, 2.0, 3.0, 3.0]), "prior_y[0]"),
    (dict(pz=[1.0, 2.0, 3.0, -np.inf]), "prior_z[3]"),
    (dict(gammas=None), "gammas is NULL"),
    (dict(leg_iters=None), "leg_iters is NULL"),
    (dict(gammas=[[0.125] * 4, [0.0, np.nan, 0.0, 0.0]]), "gammas[1][1]"),
    (dict(gammas=[[0.125] * 4, [0.0, 0.0, 1.0, 0.0]]), "gammas[1][2]"),
    (dict(gammas=[[-1.0, 0.0, 0.0, 0.0], [0.0] * 4]), "gammas[0][0]"),
    (dict(gammas=[[0.0] * 4, [0.0, 0.0, 0.0, np.inf]]), "gammas[1][3]"),
    (dict(legs=0), "legs"),
    (dict(legs=-3), "legs"),
    (dict(leg_iters=[5, -1]), "leg_iters[1]"),
    (dict(leg_iters=[2 ** 31 - 1, 1]), "INT32_MAX"),
    (dict(stop_after=-1), "stop_after"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=-0.25), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(clip=float("inf")), "clip"),
    (dict(clip=-1.0), "clip"),
    (dict(clip=float("nan")), "clip"),
    (dict(variant=3), "kernel_variant"),
    (dict(variant=-1), "kernel_variant"),
    (dict(hx=None), "hx"),
    (dict(hz=None), "hz"),
    (dict(hx=(0, [0, 0, 0, 0, 0], [])), "hx"),                       # rx < 1
    (dict(hz=(0, [0, 0, 0, 0, 0], [])), "hz"),                       # rz < 1
    (dict(hz=(2, [0, 2, 2, 3, 4], [1, 0, 1, 1])), "ascending"),      # unsorted CSC on the Hz side
    (dict(hx=(1, [0, 1, 2, 3, 4], [0, 0, 1, 0])), "hx"),             # a row out of range on the Hx side
    (dict(hz=(2, [0, 1, 2, 3, 3], [0, 0, 1, 1])), "hz"),             # colptr[n] != nnz
    (dict(n=-1), "n"),
])
def test_create_rejects_bad_arguments_before_any_device_work(change, word):
    st, msg = _create(**{**GOOD, **change})
    assert st == INVALID and word in msg, (st, msg)


def test_create_defaults_edges_and_null_handles():
    """Validation passes, and what answers then is the device lookup: LDPC_OK with a GPU, LDPC_ERR_NO_DEVICE without."""
    for kw in (dict(), dict(alpha=0.0, clip=0.0, stop_after=0), dict(opts=False), dict(leg_iters=[0, 0]), dict(leg_iters=[2 ** 31 - 1, 0]),
               dict(stop_after=7), dict(gammas=[[0.0] * 4, [np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(0)), 0.0, 0.0]])):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (OK, NO_DEVICE), (st, msg)
        if ldpc._capi.lib().ldpc_device_count() == 0:
            assert st == NO_DEVICE
    L = ldpc._capi.lib()
    assert L.ldpc_pauli_relay_kernel(None) == 0 and L.ldpc_pauli_relay_tile_syndromes(None) == 0
    assert L.ldpc_pauli_relay_last_grid(None) == 0 and L.ldpc_pauli_relay_destroy(None) == 0
    assert L.ldpc_pauli_relay_decode_batch(None, 1, None, None, None, None, None, None, None, None) == INVALID
    assert L.ldpc_pauli_relay_decode_batch_device(None, 1, None, None, None, None, None, None, None, None, None) == INVALID
    assert "NULL" in L.ldpc_last_error().decode()


# ---- the Python constructor's own refusals ---------------------------------------------------------------------------------

HX4 = np.array([[1, 1, 1, 1]], dtype=np.uint8)
HZ4 = np.array([[1, 1, 0, 0], [0, 0, 1, 1]], dtype=np.uint8)


def test_constructor_refusals():
    D = ldpc.PauliRelayMinSumDecoder
    for kw in (dict(p=None), dict(p=0.03, pauli_probs=np.full((4, 3), 0.01))):
        with pytest.raises(TypeError):
            D(HX4, HZ4, kw.pop("p"), 10, **kw)
    for kw in (dict(max_iters=10.0), dict(max_iters=True), dict(leg_iters=2.0), dict(legs=2.0), dict(stop_after=1.0), dict(stop_after=False)):
        args = {"max_iters": 10, **kw}
        with pytest.raises(TypeError):
            D(HX4, HZ4, 0.03, args.pop("max_iters"), **args)
    for kw in (dict(max_iters=-1), dict(leg_iters=-1), dict(legs=0), dict(stop_after=0), dict(gamma0=1.0), dict(gamma_range=(-1.0, 0.5)),
               dict(gamma_range=(0.5, 0.2)), dict(gammas=np.zeros((9, 3))), dict(gammas=np.zeros((8, 4))),
               dict(pauli_probs=[[0.0, 0.1, 0.1]] * 4, p=None), dict(pauli_probs=[[0.1, 0.1, 0.1]] * 3, p=None), dict(p=1.5)):
        args = {"p": 0.03, "max_iters": 10, **kw}
        with pytest.raises(ValueError):
            D(HX4, HZ4, args.pop("p"), args.pop("max_iters"), **args)
    with pytest.raises(AssertionError):
        D(HX4, np.array([[1, 0, 0, 0]], dtype=np.uint8), 0.03, 10)       # the checks do not commute
    with pytest.raises(AssertionError):
        D(HX4, np.array([[1, 1, 0]], dtype=np.uint8), 0.03, 10)          # other number of qubits
    for kw in (dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")), dict(kernel_variant=3),
               dict(gammas=np.full((9, 4), 1.0)), dict(max_iters=2 ** 31 - 1)):
        with pytest.raises(ldpc.LdpcError) as e:
            D(HX4, HZ4, 0.03, kw.pop("max_iters", 10), **kw)
        assert e.value.status == INVALID and e.value.message


def test_constructor_hands_over_what_it_documents(monkeypatch):
    """The defaults are those of RelayMinSumDecoder -- 9 legs of 30, 20, ... iterations, leg 0 at 0.125, legs 1... drawn
    from default_rng(0) -- and the priors those of PauliMinSumDecoder; without a device the library answers
    LDPC_ERR_NO_DEVICE after it has accepted the arguments, so they are read off a stub."""
    seen = {}

    class Stub:
        def __getattr__(self, name):
            def call(*a):
                seen[name] = a
                return 0
            return call

    monkeypatch.setattr(ldpc._capi, "lib_for", lambda *_: Stub())
    d = ldpc.PauliRelayMinSumDecoder(HX4, HZ4, 0.06, device=0)
    assert (d.max_iters, d.legs, d.stop_after, d.alpha, d.clip, d.n, d.rows_x, d.rows_z) == (30, 9, 1, 0.75, 1e6, 4, 1, 2)
    assert d.leg_iters.tolist() == [30] + [20] * 8 and d.leg_iters.dtype == np.int32
    want = np.empty((9, 4), dtype=np.float32)
    want[0] = np.float32(0.125)
    want[1:] = np.random.default_rng(0).uniform(-0.24, 0.66, (8, 4)).astype(np.float32)
    assert np.array_equal(d.gammas.view(np.int32), want.view(np.int32))
    pr = depolarizing_priors(4, 0.06)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((d.prior_x, d.prior_y, d.prior_z), pr))
    a = seen["ldpc_pauli_relay_create"]
    assert a[0] == 4 and a[3:6] == (d.prior_x.ctypes.data, d.prior_y.ctypes.data, d.prior_z.ctypes.data)
    assert a[6:9] == (9, d.gammas.ctypes.data, d.leg_iters.ctypes.data)
    assert (d.sparse_Hx != sp.csc_matrix(HX4)).nnz == 0 and (d.sparse_Hz != sp.csc_matrix(HZ4)).nnz == 0 and d.info().device == 0
    g = np.full((2, 4), 0.25, dtype=np.float32)
    d = ldpc.PauliRelayMinSumDecoder(HX4, HZ4, None, 7, pauli_probs=np.full((4, 3), 0.01), legs=2, leg_iters=3, gammas=g, stop_after=4, device=0)
    assert seen["ldpc_pauli_relay_create"][6] == 2 and d.leg_iters.tolist() == [7, 3] and np.array_equal(d.gammas, g) and d.stop_after == 4


# ---- the model ----------------------------------------------------------------------------------------------------------

def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_model_hand_checked_case():
    """The 2-qubit case of tests/test_pauli_cpu.py -- Hx = Hz = [1 1], priors 2 (qubit 0) and 1 (qubit 1) in all three
    tables, alpha 0.5, sx = 1, sz = 0 -- extended by one leg: leg 0 at gamma = 0, leg 1 at gamma = 0.5, one iteration each,
    stop_after = 2.
    Leg 0 is the Pauli rule (Lambda = the prior): M = ((2.5, 2), (2, 1), (1.5, 0)), qubit 1 is Z: the first solution, of
    weight qZ[1] = 65536.  Leg 1 starts from this M: g0 = 0.5 * prior = (1, 0.5), c = +0, T = +0;
    LambdaX = (1 + 1.25, 0.5 + 1) = (2.25, 1.5), LambdaY = (1 + 1, 0.5 + 0.5) = (2, 1), LambdaZ = (1 + 0.75, 0.5 + 0) = (1.75, 0.5) = G.
    The Hx row: u = min(GY, GZ) = (1.75, 0.5), w = +0, b = (1.75, 0.5), m1 = 0.5 at a = 1, m2 = 1.75, par = 1: c = (-0.25, -0.875).
    The Hz row: u = min(GY, GX) = (2, 1), m1 = 1 at a = 1, m2 = 2, par = 0: c = (0.5, 1).  TZ = (-0.25, -0.875), TX = (0.5, 1).
    With Lambda from the old M: MX = (2.75, 2.5), MZ = (1.5, -0.375), MY = ((2 + 0.5) - 0.25, (1 + 1) - 0.875) = (2.25, 1.125):
    qubit 1 is Z again: the second solution, of equal weight -- the tie keeps the first -- and the syndrome stops."""
    H = np.array([[1, 1]], dtype=np.uint8)
    pr = np.array([2.0, 1.0], dtype=np.float32)
    g = np.array([[0.0, 0.0], [0.5, 0.5]], dtype=np.float32)
    m = PauliRelayModel(H, H, (pr, pr, pr), g, [1, 1], alpha=0.5, stop_after=2)
    assert m.q[2].tolist() == [131072, 65536] and m.g0[0].tolist() == [[2.0, 1.0], [1.0, 0.5]]
    gx, gz, conv, its, sol, M = m.decode([[1]], [[0]])
    assert gx.tolist() == [[0, 0]] and gz.tolist() == [[0, 1]] and conv.tolist() == [1] and its.tolist() == [2] and sol.tolist() == [2]
    assert M.tolist() == [[[2.75, 2.5], [2.25, 1.125], [1.5, -0.375]]]
    assert (gx.dtype, gz.dtype, conv.dtype, its.dtype, sol.dtype, M.dtype) == (np.uint8, np.uint8, np.uint8, np.int32, np.int32, np.float32)
    # stop_after = 1: leg 0 alone, the Pauli result
    gx, gz, conv, its, sol, M = PauliRelayModel(H, H, (pr, pr, pr), g, [1, 1], alpha=0.5).decode([[1]], [[0]])
    assert gz.tolist() == [[0, 1]] and its.tolist() == [1] and sol.tolist() == [1] and M.tolist() == [[[2.5, 2.0], [2.0, 1.0], [1.5, 0.0]]]
    # a skipped leg in front changes nothing; every leg skipped gives zeros
    skip = PauliRelayModel(H, H, (pr, pr, pr), np.vstack([g[1:], g]), [0, 1, 1], alpha=0.5, stop_after=2).decode([[1]], [[0]])
    assert skip[5].tolist() == [[[2.75, 2.5], [2.25, 1.125], [1.5, -0.375]]] and skip[3].tolist() == [2]
    none = PauliRelayModel(H, H, (pr, pr, pr), g, [0, 0], alpha=0.5).decode([[1], [0]], [[0], [1]])
    assert all(not x.any() for x in none) and none[5].shape == (2, 3, 2) and none[3].dtype == np.int32


@functools.lru_cache(maxsize=None)
def bb72():
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    Hx, Hz = sp.csc_matrix(np.asarray(Hx) != 0), sp.csc_matrix(np.asarray(Hz) != 0)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    return Hx, Hz, Lx, Lz


def default_gammas(n=72, legs=9):
    g = np.empty((legs, n), dtype=np.float32)
    g[0] = np.float32(0.125)
    g[1:] = np.random.default_rng(0).uniform(-0.24, 0.66, (legs - 1, n)).astype(np.float32)
    return g


DEFAULT_LEGS = [30] + [20] * 8


@functools.lru_cache(maxsize=None)
def trials(p):
    """The 400 trials of css_trials_model's sampler at seed 0 and their syndromes.  Never written to."""
    Hx, Hz, _, _ = bb72()
    ex, ez = cm.sample(72, 400, p, seed=0)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    for x in (ex, ez, sx, sz):
        x.setflags(write=False)
    return ex, ez, sx, sz


@functools.lru_cache(maxsize=None)
def relay_case(p, stop_after):
    """The model at RelayMinSumDecoder's Python defaults on the 400 trials at p.  Computed once, never written to."""
    Hx, Hz, _, _ = bb72()
    _, _, sx, sz = trials(p)
    out = PauliRelayModel(Hx, Hz, depolarizing_priors(72, p), default_gammas(), DEFAULT_LEGS, stop_after=stop_after).decode(sx, sz)
    for x in out:
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("p", [0.06, 0.09])
def test_one_leg_at_gamma_zero_is_the_pauli_min_sum_model(p):
    """The consequence the header states, on the models: every output bit, the three planes included."""
    Hx, Hz, _, _ = bb72()
    _, _, sx, sz = trials(p)
    pr = depolarizing_priors(72, p)
    gx, gz, conv, its, G = PauliMinSumModel(Hx, Hz, pr, 30).decode(sx, sz)
    assert 0 < conv.sum() < 400 and len(set(its.tolist())) > 3
    one = PauliRelayModel(Hx, Hz, pr, np.zeros((1, 72), dtype=np.float32), [30]).decode(sx, sz)
    assert _same(one, (gx, gz, conv, its, conv.astype(np.int32), G))
    # zero-iteration legs around it are skipped
    more = PauliRelayModel(Hx, Hz, pr, np.zeros((3, 72), dtype=np.float32), [0, 30, 0]).decode(sx, sz)
    assert _same(more, one)


@pytest.mark.parametrize("p, stop_after, counts, mean_iters, max_iters", [
    (0.06, 1, [400, 19, 0, 19, 9, 14], 5.1025, 64),
    (0.06, 3, [400, 18, 0, 18, 9, 13], 10.855, 93),
    (0.09, 1, [400, 88, 0, 77, 52, 51], 11.77, 89),
    (0.09, 3, [400, 84, 0, 75, 51, 49], 22.9175, 169),
])
def test_bb72_statistical_pin(p, stop_after, counts, mean_iters, max_iters):
    """BB-72, the 400 model trials, RelayMinSumDecoder's defaults (README): every syndrome is reproduced, and
    the logical failures fall from the Pauli min-sum's 20 (0.06) and 91 (0.09)."""
    Hx, Hz, Lx, Lz = bb72()
    ex, ez, sx, sz = trials(p)
    gx, gz, conv, its, sol, M = relay_case(p, stop_after)
    _, got = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    print(f"p {p} stop_after {stop_after}: counts {got.tolist()} converged {int(conv.sum())} iterations {its.mean()} / {int(its.max())}")
    assert got.tolist() == counts and int(conv.sum()) == 400
    assert float(its.mean()) == mean_iters and int(its.max()) == max_iters
    assert (sol >= 1).all() and (sol <= stop_after).all() and (stop_after == 1 or (sol == stop_after).any())
    rx, rz = cm.syndromes(Hx, Hz, gx, gz)
    assert np.array_equal(rx, sx) and np.array_equal(rz, sz)


@pytest.mark.parametrize("p, counts, converged, mean_iters", [
    (0.06, [400, 22, 10, 20, 9, 15], 390, 4.3625),
    (0.09, [400, 96, 53, 91, 64, 60], 347, 9.4675),
])
def test_bb72_pauli_min_sum_rows_of_the_comparison(p, counts, converged, mean_iters):
    Hx, Hz, Lx, Lz = bb72()
    ex, ez, sx, sz = trials(p)
    gx, gz, conv, its, _ = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, p), 30).decode(sx, sz)
    _, got = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    assert got.tolist() == counts and int(conv.sum()) == converged and float(its.mean()) == mean_iters and int(its.max()) == 30


def test_a_stopped_column_is_frozen():
    """Lengthening the later legs changes nothing for a column that stopped in leg 0, and a column does not depend on its
    neighbours."""
    Hx, Hz, _, _ = bb72()
    _, _, sx, sz = trials(0.09)
    sx, sz = sx[:120], sz[:120]
    pr, g = depolarizing_priors(72, 0.09), default_gammas(legs=4)
    short = PauliRelayModel(Hx, Hz, pr, g, [6, 4, 4, 4], stop_after=1).decode(sx, sz)
    long = PauliRelayModel(Hx, Hz, pr, g, [6, 9, 9, 9], stop_after=1).decode(sx, sz)
    early = (short[2] != 0) & (short[3] <= 6)
    assert 0 < early.sum() < 120 and ((short[2] != 0) & (short[3] > 6)).any() and (short[2] == 0).any()
    assert _same(tuple(x[early] for x in short), tuple(x[early] for x in long))
    later = ~early
    assert (short[5][later].view(np.int32) != long[5][later].view(np.int32)).any()      # the others went on
    for c in (int(np.nonzero(early)[0][0]), int(np.nonzero(short[2] == 0)[0][0]), int(np.nonzero((short[2] != 0) & (short[3] > 6))[0][0])):
        assert _same(PauliRelayModel(Hx, Hz, pr, g, [6, 4, 4, 4]).decode(sx[c:c + 1], sz[c:c + 1]), tuple(x[c:c + 1] for x in short)), c
    # with stop_after = 3 a column that found a solution and went on holds the lightest of its solutions, not the decision
    # on the M it ended with; a column without a solution holds that decision
    three = PauliRelayModel(Hx, Hz, pr, g, [6, 4, 4, 4], stop_after=3).decode(sx, sz)
    ex, ez = PauliMinSumModel._decide(three[5][:, 0], three[5][:, 1], three[5][:, 2])
    differs = ((three[0] != 0) != ex).any(axis=1) | ((three[1] != 0) != ez).any(axis=1)
    assert differs.any() and (three[4] == 0).any() and not differs[three[4] == 0].any()
