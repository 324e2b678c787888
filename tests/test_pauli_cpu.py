"""Joint X/Z (Pauli) min-sum decoder without a GPU: the planner sizes (csrc/tile_plan.hpp pauli_tile_plan through
ldpc_debug_pauli_tile_plan) at hand-computed shapes, the argument validation of ldpc_pauli_minsum_create (which answers
before any device work), the Python constructor's own refusals, the numpy model of the rule (tests/pauli_model.py) on
properties that follow from the rule alone, and one statistical comparison on the models: the joint decoder against the
two independent min-sum decoders it replaces."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import ldpcdecoders_jl_amd as ldpc
from minsum_model import MinSumModel, llr_of_probs
from pauli_model import PauliMinSumModel, depolarizing_priors, pauli_priors

INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 5


# ---- the planner --------------------------------------------------------------------------------------------------------

def _plan(s, n, rec_words, variant=0):
    L = ldpc._capi.lib()
    tier, S, state = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.ldpc_debug_pauli_tile_plan(s, n, rec_words, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(state))
    return st, tier.value, S.value, state.value


@pytest.mark.parametrize("s, n, rec_words, variant, want", [
    # BB-72: 36 + 36 checks of degree 6 -> 288 record words; 4 (144 + 288) + 72 = 1800 B a syndrome; 64 of them are
    # 115200 B > 79 KiB = 80896 B, 32 of them 57600 B
    (72, 72, 288, 0, (1, 32, 57600)),
    (72, 72, 288, 1, (1, 32, 57600)),
    (72, 72, 288, 2, (2, 64, 115200)),
    # the hypergraph product of two 3-bit repetition checks: n = 13, 6 + 6 checks of degree <= 3 -> 48 words;
    # 4 (26 + 48) + 12 = 308 B a syndrome, 64 of them 19712 B
    (12, 13, 48, 0, (1, 64, 19712)),
    # 4 (450 + 864) + 216 = 5472 B a syndrome: 16 of them 87552 B > 80896 B, 8 of them 43776 B
    (216, 225, 864, 0, (1, 8, 43776)),
    # 4 (8000 + 16000) + 4000 = 100000 B a syndrome: past 79 KiB, inside 159 KiB = 162816 B; rounded up to 256: 100096
    (4000, 4000, 16000, 0, (1, 1, 100096)),
    # 500000 B a syndrome: the unlimited tier by size, 64 syndromes a slot
    (20000, 20000, 80000, 0, (2, 64, 32000000)),
    # an empty graph still has its syndrome bytes: 64 * 3 = 192 B -> 256
    (3, 0, 0, 0, (1, 64, 256)),
])
def test_planner_sizes_at_hand_computed_shapes(s, n, rec_words, variant, want):
    assert _plan(s, n, rec_words, variant) == (0,) + want


def test_planner_refusals():
    assert _plan(20000, 20000, 80000, 1)[0] == UNSUPPORTED          # forced on-chip, nothing fits
    assert _plan(72, 72, 288, 3)[0] == INVALID and _plan(-1, 72, 288)[0] == INVALID and _plan(72, 72, -1)[0] == INVALID
    assert _plan(72, 1 << 28, 0)[0] == INVALID
    L = ldpc._capi.lib()
    assert L.ldpc_debug_pauli_tile_plan(72, 72, 288, 0, None, None, None) == 0   # every out pointer may be NULL


# ---- symbols ------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("ldpc_pauli_minsum_create", "ldpc_pauli_minsum_destroy", "ldpc_pauli_minsum_kernel", "ldpc_pauli_minsum_tile_syndromes",
               "ldpc_pauli_minsum_last_grid", "ldpc_pauli_minsum_decode_batch", "ldpc_pauli_minsum_decode_batch_device")


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_declared_and_exported(experiments):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ldpc_mi355x.h")).read(), flags=re.S)
    lib = ldpc._capi.lib(experiments)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "ldpc_debug_pauli_tile_plan" in ldpc._capi.DEBUG_SYMBOLS and hasattr(lib, "ldpc_debug_pauli_tile_plan")
    assert lib.ldpc_abi_version() == 4
    assert ctypes.sizeof(ldpc._capi.PauliMinSumOptions) == 64
    assert ldpc.PauliMinSumDecoder is ldpc.pauli.PauliMinSumDecoder and callable(ldpc.run_css_joint_trials)


# ---- ldpc_pauli_minsum_create validates before it looks for a device -------------------------------------------------------

def _pattern(rows, colptr, rowval, keep):
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    keep += [colptr, rowval]
    pat = ldpc._capi.CSSPattern()
    pat.rows, pat.nnz, pat.colptr, pat.rowval = rows, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data
    return pat


# n = 4: Hx = [1 1 1 1], Hz = [1 1 0 0; 0 0 1 1]
GOOD = dict(n=4, hx=(1, [0, 1, 2, 3, 4], [0, 0, 0, 0]), hz=(2, [0, 1, 2, 3, 4], [0, 0, 1, 1]),
            px=[3.0, 3.0, 3.0, 3.0], py=[3.5, 3.0, 3.0, -1.0], pz=[3.0, 2.0, 3.0, 3.0])


def _create(n, hx, hz, px, py, pz, max_iters=10, alpha=None, clip=None, variant=0, opts=True):
    L = ldpc._capi.lib()
    keep = []
    pats = [ctypes.byref(_pattern(*h, keep)) if h is not None else None for h in (hx, hz)]
    tables = [np.asarray(t, dtype=np.float32) if t is not None else None for t in (px, py, pz)]
    o = ldpc._capi.PauliMinSumOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    o.kernel_variant = variant
    h = ctypes.c_void_p()
    st = L.ldpc_pauli_minsum_create(n, pats[0], pats[1], *(t.ctypes.data if t is not None else None for t in tables), max_iters,
                                    ctypes.byref(o) if opts else None, ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_pauli_minsum_kernel(h) in (1, 2) and L.ldpc_pauli_minsum_last_grid(h) == 0
        L.ldpc_pauli_minsum_destroy(h)
    else:
        assert not h.value
    return st, msg


@pytest.mark.parametrize("change, word", [
    (dict(px=None), "prior_x"),
    (dict(py=None), "prior_y"),
    (dict(pz=None), "prior_z"),
    (dict(px=[1.0, np.nan, 3.0, 3.0]), "prior_x[1]"),
    (dict(py=[np.inf, 2.0, 3.0, 3.0]), "prior_y[0]"),
    (dict(pz=[1.0, 2.0, 3.0, -np.inf]), "prior_z[3]"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=-0.25), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(clip=float("inf")), "clip"),
    (dict(clip=-1.0), "clip"),
    (dict(clip=float("nan")), "clip"),
    (dict(variant=3), "kernel_variant"),
    (dict(variant=-1), "kernel_variant"),
    (dict(max_iters=-1), "max_iters"),
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


def test_create_defaults_and_null_handles():
    """A zeroed options struct means defaults: validation passes, and what answers then is the device lookup -- LDPC_OK
    with a GPU, LDPC_ERR_NO_DEVICE without."""
    for kw in (dict(), dict(alpha=0.0, clip=0.0), dict(opts=False), dict(max_iters=0)):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (0, NO_DEVICE), (st, msg)
    L = ldpc._capi.lib()
    assert L.ldpc_pauli_minsum_kernel(None) == 0 and L.ldpc_pauli_minsum_tile_syndromes(None) == 0
    assert L.ldpc_pauli_minsum_last_grid(None) == 0 and L.ldpc_pauli_minsum_destroy(None) == 0
    assert L.ldpc_pauli_minsum_decode_batch(None, 1, None, None, None, None, None, None, None) == INVALID
    assert L.ldpc_pauli_minsum_decode_batch_device(None, 1, None, None, None, None, None, None, None, None) == INVALID
    assert L.ldpc_pauli_minsum_decode_batch_device(None, 0, None, None, None, None, None, None, None, None) == INVALID
    h = ctypes.c_void_p(1)
    assert L.ldpc_pauli_minsum_create(4, None, None, None, None, None, 1, None, None) == INVALID   # out is NULL
    assert L.ldpc_pauli_minsum_create(4, None, None, None, None, None, 1, None, ctypes.byref(h)) == INVALID and not h.value


def test_constructor_refusals_and_priors():
    Hx = np.array([[1, 1, 1, 1]], dtype=np.uint8)
    Hz = np.array([[1, 1, 0, 0], [0, 0, 1, 1]], dtype=np.uint8)
    for kw in (dict(p=None), dict(p=0.03, pauli_probs=np.full((4, 3), 0.01))):
        with pytest.raises(TypeError):
            ldpc.PauliMinSumDecoder(Hx, Hz, kw.pop("p"), 10, **kw)
    with pytest.raises(TypeError):
        ldpc.PauliMinSumDecoder(Hx, Hz, 0.03, 10.0)
    for probs in ([[0.0, 0.1, 0.1]] * 4, [[0.4, 0.3, 0.3]] * 4, [[0.1, float("nan"), 0.1]] * 4, [[0.1, -0.2, 0.1]] * 4,
                  [[0.1, 0.1, 0.1]] * 3, [[0.1, 0.1]] * 4):
        with pytest.raises(ValueError):
            ldpc.PauliMinSumDecoder(Hx, Hz, None, 10, pauli_probs=probs)
    for p in (0.0, 1.5, (0.5, 0.5, 0.1), (0.5, 0.25, 0.25), (0.0, 0.1, 0.1)):
        with pytest.raises(ValueError):
            ldpc.PauliMinSumDecoder(Hx, Hz, p, 10)
    with pytest.raises(AssertionError):
        ldpc.PauliMinSumDecoder(Hx, np.array([[1, 0, 0, 0]], dtype=np.uint8), 0.03, 10)       # the checks do not commute
    with pytest.raises(AssertionError):
        ldpc.PauliMinSumDecoder(Hx, np.array([[1, 1, 0]], dtype=np.uint8), 0.03, 10)          # other number of qubits
    for kw in (dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")), dict(kernel_variant=3)):
        with pytest.raises(ldpc.LdpcError) as e:
            ldpc.PauliMinSumDecoder(Hx, Hz, 0.03, 10, **kw)
        assert e.value.status == INVALID and e.value.message
    # the package's own priors equal the model's, bit for bit; some of these are negative
    from ldpcdecoders_jl_amd.pauli import pauli_priors as pkg_priors

    probs = np.random.default_rng(3).uniform(1e-4, 0.3, (100, 3))
    assert np.array_equal(pkg_priors(probs).view(np.int32), pauli_priors(probs).view(np.int32)) and (pkg_priors(probs) < 0).any()
    assert pkg_priors(probs).shape == (3, 100) and pkg_priors(probs).dtype == np.float32


# ---- the model ----------------------------------------------------------------------------------------------------------

def test_model_hand_checked_case():
    """Hx = Hz = [1 1], priors 2 (qubit 0) and 1 (qubit 1) in all three tables, alpha 0.5, sx = 1, sz = 0.
    Check sweep 1: the Hx row has u = (2, 1), w = +0, b = (2, 1), m1 = 1 at a = 1, m2 = 2, par = 1: c = (-0.5, -1);
    the Hz row the same with par = 0: c = (0.5, 1).  TZ = (-0.5, -1), TX = (0.5, 1);
    GX = (2.5, 2), GY = ((2 + 0.5) - 0.5, (1 + 1) - 1) = (2, 1), GZ = (1.5, 0): qubit 0 is I (its least G, 1.5, is > 0),
    qubit 1 is Z (GZ = 0 <= 0): ez = (0, 1) reproduces sx = 1, ex = (0, 0) reproduces sz = 0."""
    H = np.array([[1, 1]], dtype=np.uint8)
    pr = np.array([2.0, 1.0], dtype=np.float32)
    gx, gz, conv, its, G = PauliMinSumModel(H, H, (pr, pr, pr), 5, alpha=0.5).decode([[1]], [[0]])
    assert gx.tolist() == [[0, 0]] and gz.tolist() == [[0, 1]] and conv[0] == 1 and its[0] == 1
    assert G.tolist() == [[[2.5, 2.0], [2.0, 1.0], [1.5, 0.0]]]
    # the mirror image: sx = 0, sz = 1 gives an X on qubit 1
    gx, gz, conv, its, G = PauliMinSumModel(H, H, (pr, pr, pr), 5, alpha=0.5).decode([[0]], [[1]])
    assert gx.tolist() == [[0, 1]] and gz.tolist() == [[0, 0]] and conv[0] == 1 and G.tolist() == [[[1.5, 0.0], [2.0, 1.0], [2.5, 2.0]]]
    # both: the Y belief of qubit 1 is (1 - 1) - 1 = -1, below GX = GZ = 0: one Y, not an X and a Z elsewhere
    gx, gz, conv, its, G = PauliMinSumModel(H, H, (pr, pr, pr), 5, alpha=0.5).decode([[1]], [[1]])
    assert gx.tolist() == [[0, 1]] and gz.tolist() == [[0, 1]] and conv[0] == 1 and G[0, :, 1].tolist() == [0.0, -1.0, 0.0]


@functools.lru_cache(maxsize=None)
def bb72():
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    Hx, Hz = sp.csc_matrix(np.asarray(Hx) != 0), sp.csc_matrix(np.asarray(Hz) != 0)
    assert Hx.shape == Hz.shape == (36, 72)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    return Hx, Hz, Lx, Lz


P, TRIALS, ITERS, SEED = 0.06, 400, 30, 0


@functools.lru_cache(maxsize=None)
def statistical_case():
    """BB-72, depolarizing 0.06, the 400 trials of css_trials_model's sampler at seed 0, 30 iterations: the joint model
    and the two independent min-sum models at the marginal rate 2 p / 3, each scored.  Computed once, never written to."""
    Hx, Hz, Lx, Lz = bb72()
    ex, ez = cm.sample(72, TRIALS, P, seed=SEED)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    joint = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, P), ITERS).decode(sx, sz)
    marginal = llr_of_probs(np.full(72, 2.0 * P / 3.0))
    side_x = MinSumModel(Hz, marginal, ITERS).decode(sz)     # Hz sees the X parts
    side_z = MinSumModel(Hx, marginal, ITERS).decode(sx)
    _, joint_counts = cm.score(Hx, Hz, Lx, Lz, joint[0], joint[1], ex, ez)
    _, indep_counts = cm.score(Hx, Hz, Lx, Lz, side_x[0], side_z[0], ex, ez)
    for x in joint + side_x + side_z + (sx, sz, ex, ez):
        x.setflags(write=False)
    conv, its = joint[2], joint[3]
    assert 0 < conv.sum() < TRIALS and len(set(its.tolist())) > 3     # equality tests on this batch are not vacuous
    return dict(sx=sx, sz=sz, ex=ex, ez=ez, joint=joint, side_x=side_x, side_z=side_z, joint_counts=joint_counts, indep_counts=indep_counts)


def test_joint_model_fails_less_often_than_two_independent_min_sums():
    """Measured with these models (README): 20 trials with a logical failure (9 X / 15 Z) and 390 converged
    under the joint rule, against 82 (43 X / 52 Z) with 345 trials in which both sides converged."""
    c = statistical_case()
    joint_conv = int(c["joint"][2].sum())
    indep_conv = int((c["side_x"][1] & c["side_z"][1]).sum())
    print(f"joint: counts {c['joint_counts'].tolist()} converged {joint_conv} mean iterations {c['joint'][3].mean():.2f}; "
          f"independent: counts {c['indep_counts'].tolist()} both converged {indep_conv}")
    assert c["joint_counts"][0] == c["indep_counts"][0] == TRIALS
    assert c["joint_counts"][3] < c["indep_counts"][3]
    # the measured values the documents quote
    assert c["joint_counts"].tolist() == [400, 22, 10, 20, 9, 15] and joint_conv == 390
    assert c["indep_counts"].tolist() == [400, 87, 55, 82, 43, 52] and indep_conv == 345


def test_model_converged_means_both_syndromes_reproduced():
    c = statistical_case()
    Hx, Hz, _, _ = bb72()
    gx, gz, conv, its, G = c["joint"]
    ok = conv != 0
    assert np.array_equal(cm.syndromes(Hx, Hz, gx, gz)[0][ok], c["sx"][ok]) and np.array_equal(cm.syndromes(Hx, Hz, gx, gz)[1][ok], c["sz"][ok])
    bad = ~ok
    mism = (cm.syndromes(Hx, Hz, gx, gz)[0][bad] != c["sx"][bad]).any(axis=1) | (cm.syndromes(Hx, Hz, gx, gz)[1][bad] != c["sz"][bad]).any(axis=1)
    assert mism.all() and (its[bad] == ITERS).all() and (its[ok] >= 1).all()
    # the outputs are the decision on the returned beliefs
    ex, ez = PauliMinSumModel._decide(G[:, 0], G[:, 1], G[:, 2])
    assert np.array_equal(ex, gx != 0) and np.array_equal(ez, gz != 0) and G.dtype == np.float32


def test_model_max_iters_zero():
    Hx, Hz, _, _ = bb72()
    out = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, P), 0).decode(np.ones((3, 36), np.uint8), np.ones((3, 36), np.uint8))
    assert all(not x.any() for x in out) and out[4].shape == (3, 3, 72) and out[4].dtype == np.float32 and out[3].dtype == np.int32


def test_model_frozen_column_does_not_change_when_max_iters_grows():
    c = statistical_case()
    Hx, Hz, _, _ = bb72()
    gx, gz, conv, its, G = c["joint"]
    short = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, P), 5).decode(c["sx"], c["sz"])
    early = (conv != 0) & (its <= 5)
    assert 0 < early.sum() < TRIALS
    assert np.array_equal(short[2] != 0, early) and np.array_equal(short[3][early], its[early]) and (short[3][~early] == 5).all()
    assert np.array_equal(short[0][early], gx[early]) and np.array_equal(short[1][early], gz[early])
    assert np.array_equal(short[4][early].view(np.int32), G[early].view(np.int32))
    assert (short[4][~early].view(np.int32) != G[~early].view(np.int32)).any()      # the others went on
    # a column does not depend on its neighbours
    one = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, P), ITERS).decode(c["sx"][7:8], c["sz"][7:8])
    assert np.array_equal(one[4][0].view(np.int32), G[7].view(np.int32)) and one[3][0] == its[7]
