"""Sliding-window decoding without a GPU: the library's plan against the model's (tests/windows_model.py), the partition
property by brute force, the model chain's identity residual = syndromes ^ H guess, the refusals, the sharing of window
decoders, the conditions that keep the GPU fixture of tests/test_gpu_windows.py from being vacuous, the refusals of
ldpc_windows_create that answer before any device work, and the table builder under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import dem_model as dm
import trials_model as tm
import windows_model as wm
from minsum_model import MinSumModel, llr_of_probs

INVALID, NO_DEVICE = 1, 2
SHAPES = [(5, 3, 1), (6, 4, 2), (4, 4, 1), (3, 5, 2)]
WINDOWS = {(5, 3, 1): 3, (6, 4, 2): 2, (4, 4, 1): 1, (3, 5, 2): 1}


@pytest.fixture(scope="module")
def bb72(ldpc):
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    return HX, ldpc.codes.css_logicals(HX, HZ)[1]


def hand_made(ldpc):
    """Seven detectors in shuffled layer order, a mechanism over three layers (2), one without a detector (3)."""
    cols = [(1, 4), (3, 4), (0, 1, 6), (), (3, 5), (0, 2), (2,), (2, 5, 6)]
    rows = [d for c in cols for d in c]
    H = sp.csc_matrix((np.ones(len(rows), dtype=np.uint8), (rows, np.repeat(np.arange(8), [len(c) for c in cols]))), shape=(7, 8))
    L = sp.csc_matrix(np.array([[0, 0, 0, 1, 0, 0, 1, 0]], dtype=np.uint8))
    dem = ldpc.DetectorErrorModel(H, L, np.linspace(0.01, 0.08, 8))
    return dem, np.array([2, 0, 3, 1, 0, 2, 1])


def _same_plan(p, windows, uncovered):
    assert len(p.windows) == len(p) == len(windows)
    for got, want in zip(p.windows, windows):
        assert (got.a, got.b) == (want["a"], want["b"])
        for f in ("det", "mech", "commit"):
            assert getattr(got, f).dtype == np.int64 and np.array_equal(getattr(got, f), want[f]), f
    assert np.array_equal(p.uncovered, uncovered)


def _partition(H, p):
    """Every mechanism with a detector is committed exactly once; after the commit of window k every uncommitted
    mechanism has all its detectors in layers >= a_{k+1}."""
    H = sp.csc_matrix(H)
    n = H.shape[1]
    count = np.zeros(n, dtype=np.int64)
    for k, w in enumerate(p.windows):
        assert np.all(np.diff(w.det) > 0) and np.all(np.diff(w.mech) > 0) and np.all(np.diff(w.commit) > 0)
        for c in w.commit:
            count[w.mech[c]] += 1
        if k + 1 < len(p.windows):
            for j in range(n):
                dets = H.indices[H.indptr[j]:H.indptr[j + 1]]
                if count[j] == 0 and dets.size:
                    assert all(p.layers[d] >= p.windows[k + 1].a for d in dets), (k, j)
    has = np.diff(H.indptr) > 0
    assert np.array_equal(count, has.astype(np.int64))


@pytest.mark.parametrize("shape", SHAPES)
def test_plan_of_the_phenomenological_model_equals_the_model(ldpc, bb72, shape):
    R, W, C = shape
    HX, logicals = bb72
    dem = ldpc.phenomenological(HX, logicals, R, 0.01, 0.02)
    layers = ldpc.phenomenological_layers(HX, R)
    assert np.array_equal(layers, np.repeat(np.arange(R), 36)) and layers.shape == (dem.num_detectors,)
    p = ldpc.window_plan(dem, layers, W, C)
    assert isinstance(p, ldpc.WindowPlan)
    _same_plan(p, *wm.plan(dem.H, layers, W, C))
    assert len(p) == WINDOWS[shape]
    _partition(dem.H, p)
    for k, w in enumerate(p.windows):
        m = p.sub_model(k)
        assert isinstance(m, ldpc.DetectorErrorModel) and m.L.shape == (0, w.mech.size)
        assert (m.H != wm.sub_matrix(dem.H, wm.plan(dem.H, layers, W, C)[0][k])).nnz == 0
        assert np.array_equal(m.rates, dem.rates[w.mech])
    if len(p) == 1:
        assert p.sub_model(0) == ldpc.DetectorErrorModel(dem.H, None, dem.rates)


def test_plan_of_a_hand_made_model(ldpc):
    dem, layers = hand_made(ldpc)
    for W in range(1, 6):
        for C in range(1, W + 1):
            p = ldpc.window_plan(dem, layers, W, C, strict=False)
            _same_plan(p, *wm.plan(dem.H, layers, W, C, strict=False))
            _partition(dem.H, p)
            assert p.uncovered.tolist() == [3]
    p = ldpc.window_plan(dem, layers, 3, 1)                       # the three-layer mechanism just fits
    assert [(w.a, w.b) for w in p.windows] == [(0, 3), (1, 4)]
    assert p.windows[0].det.tolist() == [0, 1, 3, 4, 5, 6] and p.windows[0].mech.tolist() == [0, 1, 2, 4, 5, 7]
    assert p.windows[0].commit.tolist() == [0, 1, 2] and p.windows[1].mech.tolist() == [4, 5, 6, 7]
    # the truncated column: mechanism 5 (detectors 0 and 2, layers 2 and 3) keeps detector 0 alone in window 0
    assert p.sub_model(0).H[:, 4].nnz == 1
    for W, C in ((3, 2), (2, 1), (2, 2)):                          # ... and no longer fits
        with pytest.raises(ValueError):
            ldpc.window_plan(dem, layers, W, C)
        with pytest.raises(ValueError):
            wm.plan(dem.H, layers, W, C)


def test_refusals_of_the_plan(ldpc, bb72):
    HX, logicals = bb72
    dem = ldpc.phenomenological(HX, logicals, 4, 0.01, 0.02)
    layers = ldpc.phenomenological_layers(HX, 4)
    for W, C in ((0, 1), (3, 0), (2, 3), (-1, -1)):
        with pytest.raises(ValueError):
            ldpc.window_plan(dem, layers, W, C)
    with pytest.raises(ValueError):
        ldpc.window_plan(dem, layers[:-1], 3, 1)
    bad = layers.copy()
    bad[5] = -1
    with pytest.raises(ValueError):
        ldpc.window_plan(dem, bad, 3, 1)
    for W, C in ((2, 2), (1, 1), (3, 3)):                          # phenomenological: strict means width > commit
        with pytest.raises(ValueError):
            ldpc.window_plan(dem, layers, W, C)
        p = ldpc.window_plan(dem, layers, W, C, strict=False)
        _same_plan(p, *wm.plan(dem.H, layers, W, C, strict=False))
        _partition(dem.H, p)
    assert len(ldpc.window_plan(dem, layers, 4, 4)) == 1           # one window: nothing is committed early
    with pytest.raises(ValueError):
        ldpc.phenomenological_layers(HX, 0)


@pytest.fixture(scope="module")
def fixture_chain(ldpc, bb72):
    """The fixture of tests/test_gpu_windows.py through the model chain around MinSumModel."""
    HX, logicals = bb72
    dem = ldpc.phenomenological(HX, logicals, 5, 0.01, 0.02)
    syn = tm.syndromes(dem.H, dm.sample(dem.rates, 200, 7, 0))
    layers = ldpc.phenomenological_layers(HX, 5)
    windows, uncovered = wm.plan(dem.H, layers, 3, 1)

    def decode_of(H, rates):
        model = MinSumModel(H, llr_of_probs(rates), 30)
        return lambda s: model.decode(s)[:2]
    return dem, syn, windows, wm.chain(dem.H, dem.rates, windows, uncovered, decode_of, syn), decode_of


def test_the_gpu_fixture_is_not_vacuous(fixture_chain):
    dem, syn, windows, (guess, conv, residual, stats), decode_of = fixture_chain
    assert [(w["det"].size, w["mech"].size) for w in windows] == [(108, 324), (108, 324), (108, 288)]
    assert stats[-1] == dict(decoders=2)                           # 3 windows over 2 decoders
    assert [s["unconverged"] for s in stats[:3]] == [32, 26, 1]
    assert [s["flipped"] for s in stats[:2]] == [118, 97]          # commits that flip later detectors
    assert int(conv.sum()) == 150
    assert int((~residual.any(axis=1)).sum()) == 197
    assert np.array_equal(residual, syn ^ tm.syndromes(dem.H, guess))
    assert guess.max() <= 1
    one_shot = decode_of(dem.H, dem.rates)(syn)[0]
    assert int((one_shot != guess).any(axis=1).sum()) == 3


def test_the_model_chain_keeps_the_identity_on_the_hand_made_model(ldpc):
    dem, layers = hand_made(ldpc)
    rng = np.random.default_rng(3)
    syn = rng.integers(0, 2, size=(9, 7), dtype=np.uint8)
    for W, C, strict in ((3, 1, True), (2, 1, False), (1, 1, False), (5, 2, True)):
        windows, uncovered = wm.plan(dem.H, layers, W, C, strict=strict)

        def decode_of(H, rates):
            return lambda s: (rng.integers(0, 4, size=(s.shape[0], H.shape[1]), dtype=np.uint8), rng.integers(0, 2, size=s.shape[0], dtype=np.uint8))
        guess, conv, residual, _ = wm.chain(dem.H, dem.rates, windows, uncovered, decode_of, syn)
        assert guess.max() <= 1 and np.all(guess[:, 3] == 0)
        assert np.array_equal(residual, syn ^ tm.syndromes(dem.H, guess))


def test_windows_of_equal_model_share_a_decoder(ldpc, bb72, monkeypatch):
    """(5, 3, 1): three windows, two distinct models -- make_decoder is called twice.  The window step handle is replaced,
    so that the constructor runs without a device."""
    HX, logicals = bb72
    dem = ldpc.phenomenological(HX, logicals, 5, 0.01, 0.02)
    windows_py = __import__("importlib").import_module(ldpc.SlidingWindowDecoder.__module__)

    class NoStep:
        def __init__(self, *a, **k):
            pass

        def close(self):
            pass

    monkeypatch.setattr(windows_py, "WindowStep", NoStep)
    made = []

    class Fake:
        def __init__(self, m):
            made.append(m)

        def close(self):
            pass

    dec = ldpc.SlidingWindowDecoder(dem, ldpc.phenomenological_layers(HX, 5), 3, 1, Fake, device=None)
    assert len(made) == 2 and len(dec.decoders) == 2 and dec.window_decoder == [0, 0, 1]
    assert made[0].H.shape == (108, 324) and made[1].H.shape == (108, 288)
    assert dec.sparse_H is dem.H and dec.per is None and len(dec.plan) == 3 and dec.info().windows == 3
    dec.close()
    # different rates in the second window: three models
    rates = dem.rates.copy()
    rates[80] = 0.3                                                # a data mechanism of round 1
    made.clear()
    dec = ldpc.SlidingWindowDecoder(ldpc.DetectorErrorModel(dem.H, dem.L, rates), ldpc.phenomenological_layers(HX, 5), 3, 1, Fake)
    assert dec.window_decoder == [0, 1, 2] and len(made) == 3
    dec.close()


def _create(lib, H, det, mech, commit, out=None):
    H = sp.csc_matrix(H)
    H.sort_indices()
    colptr, rowval = H.indptr.astype(np.int64), H.indices.astype(np.int64)

    def lists(x):
        ptr = np.zeros(len(x) + 1, dtype=np.int64)
        np.cumsum([len(v) for v in x], out=ptr[1:])
        return ptr, np.array([i for v in x for i in v] + [0], dtype=np.int64)   # (never empty: a pointer to hand over)
    dp, di = lists(det)
    mp, mi = lists(mech)
    cp, ci = lists(commit)
    h = ctypes.c_void_p() if out is None else out
    st = lib.ldpc_windows_create(H.shape[0], H.shape[1], int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, len(det),
                                 dp.ctypes.data, di.ctypes.data, mp.ctypes.data, mi.ctypes.data, cp.ctypes.data, ci.ctypes.data,
                                 None, ctypes.byref(h))
    return st, h, lib.ldpc_last_error().decode()


def test_create_refuses_before_any_device_work(ldpc):
    lib = ldpc._capi.lib()
    for sym in ("ldpc_windows_create", "ldpc_windows_destroy", "ldpc_windows_count", "ldpc_windows_gather_device",
                "ldpc_windows_commit_device"):
        assert sym in ldpc._capi.EXPORTED_SYMBOLS and getattr(lib, sym)
    dem, layers = hand_made(ldpc)
    p = ldpc.window_plan(dem, layers, 3, 1)
    det, mech, commit = ([w.det.tolist() for w in p.windows], [w.mech.tolist() for w in p.windows], [w.commit.tolist() for w in p.windows])

    def changed(lists, k, i, value):
        out = [list(v) for v in lists]
        out[k][i] = value
        return out
    for args, needle in (
            ((changed(det, 1, 2, 7), mech, commit), "window 1: det_idx[2]"),                 # out of range
            ((changed(det, 0, 0, -1), mech, commit), "window 0: det_idx[0]"),
            ((det, changed(mech, 1, 3, 8), commit), "window 1: mech_idx[3]"),
            ((det, mech, changed(commit, 0, 2, 6)), "window 0: commit_idx[2]"),              # a position, not an index
            ((changed(det, 0, 1, 0), mech, commit), "window 0: det_idx[1]"),                 # not distinct
            ((det, changed(mech, 1, 1, 4), commit), "window 1: mech_idx[1]"),                # not ascending
            ((det, mech, changed(commit, 0, 1, 0)), "window 0: commit_idx[1]"),
            ((det, [mech[0], mech[0]], [commit[0], [0]]), "window 1: commit_idx[0]: mechanism 0 is committed by window 0"),
    ):
        st, h, msg = _create(lib, dem.H, *args)
        assert st == INVALID and not h.value and needle in msg, (needle, msg)
    h = ctypes.c_void_p()
    one = np.zeros(2, dtype=np.int64)
    assert lib.ldpc_windows_create(1, 1, 0, one.ctypes.data, one.ctypes.data, 1, None, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data, None, ctypes.byref(h)) == INVALID
    assert lib.ldpc_windows_create(1, 1, 0, one.ctypes.data, one.ctypes.data, -1, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data, one.ctypes.data, None, ctypes.byref(h)) == INVALID
    assert lib.ldpc_windows_create(1, 1, 0, one.ctypes.data, one.ctypes.data, 0, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data, one.ctypes.data, None, None) == INVALID
    falling = np.array([1, 0], dtype=np.int64)                     # a pattern ldpc_bp_create rejects: rows 1, 0 in a column
    two = np.array([0, 2], dtype=np.int64)
    assert lib.ldpc_windows_create(2, 1, 2, two.ctypes.data, falling.ctypes.data, 0, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data, one.ctypes.data, None, ctypes.byref(h)) == INVALID
    # the handle-less answers
    assert lib.ldpc_windows_destroy(None) == 0 and lib.ldpc_windows_count(None) == 0
    assert lib.ldpc_windows_gather_device(None, 0, 1, None, None, None) == INVALID and "handle" in lib.ldpc_last_error().decode()
    assert lib.ldpc_windows_commit_device(None, 0, 1, None, None, None, None, None, None, None) == INVALID
    # a good plan: a handle where there is a device, LDPC_ERR_NO_DEVICE where there is none (no CPU fallback)
    st, h, msg = _create(lib, dem.H, det, mech, commit)
    if lib.ldpc_device_count() == 0:
        assert st == NO_DEVICE and not h.value, msg
        with pytest.raises(ldpc.LdpcError) as ei:
            ldpc.WindowStep(dem.H, det, mech, commit)
        assert ei.value.status == NO_DEVICE
    else:
        assert st == 0 and lib.ldpc_windows_count(h) == 2
        assert lib.ldpc_windows_destroy(h) == 0


def test_window_tables_under_sanitizers(tmp_path):
    """window_plan.cpp built with AddressSanitizer + UBSan (CPU only) and driven by tests/native/window_plan_sanitize.cpp:
    the tables of the phenomenological plans, of a hand-made model at every (width, commit) and the refusals."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "window_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-o", exe, os.path.join(root, "tests", "native", "window_plan_sanitize.cpp"),
                           os.path.join(root, "ldpcdecoders.jl_amd", "csrc", "window_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
