"""Stabilizer (non-CSS) min-sum decoder without a GPU: the planner sizes (csrc/tile_plan.hpp stab_tile_plan through
ldpc_debug_stab_tile_plan) at hand-computed shapes, the symbols, the argument validation of ldpc_stab_minsum_create (which
answers before any device work), the Python constructor's own refusals, the code helpers of codes.py, the numpy model of
the rule (tests/stab_model.py) on properties that follow from the rule alone, and one statistical comparison on the
models: the joint rule against binary min-sum on the symplectic matrix [Sz | Sx], which it replaces."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import ldpcdecoders_jl_amd as ldpc
import trials_model as tm
from ldpcdecoders_jl_amd import codes
from minsum_model import MinSumModel, llr_of_probs
from pauli_model import PauliMinSumModel, depolarizing_priors
from stab_model import StabMinSumModel, symplectic_syndromes

INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 5


# ---- the planner --------------------------------------------------------------------------------------------------------

def _plan(r, n, rec_words, variant=0):
    L = ldpc._capi.lib()
    tier, S, state = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.ldpc_debug_stab_tile_plan(r, n, rec_words, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(state))
    return st, tier.value, S.value, state.value


@pytest.mark.parametrize("r, n, rec_words, variant, want", [
    # deformed BB-72: 72 checks of degree 6 -> 288 record words; 4 (216 + 288) + 72 = 2088 B a syndrome; 64 of them are
    # 133632 B > 79 KiB = 80896 B, 32 of them 66816 B
    (72, 72, 288, 0, (1, 32, 66816)),
    (72, 72, 288, 1, (1, 32, 66816)),
    (72, 72, 288, 2, (2, 64, 133632)),
    # the five-qubit code: 4 checks of degree 4 -> 16 words; 4 (15 + 16) + 4 = 128 B a syndrome
    (4, 5, 16, 0, (1, 64, 8192)),
    # XZZX d = 5: 40 checks of degree 3 or 4 -> 160 words; 4 (123 + 160) + 40 = 1172 B a syndrome, 64 of them 75008 B
    (40, 41, 160, 0, (1, 64, 75008)),
    # HGP of two (12, 4, 3) matrices: 4 (675 + 864) + 216 = 6372 B a syndrome: 16 of them 101952 B > 80896 B, 8 of them
    # 50976 B, which the rounding up to 256 of every state size in the family makes 51200
    (216, 225, 864, 0, (1, 8, 51200)),
    # 4 (60000 + 80000) + 20000 = 580000 B a syndrome: the unlimited tier by size
    (20000, 20000, 80000, 0, (2, 64, 37120000)),
])
def test_planner_sizes_at_hand_computed_shapes(r, n, rec_words, variant, want):
    assert _plan(r, n, rec_words, variant) == (0,) + want
    assert want[2] % 256 == 0 and 0 <= want[2] - (4 * (3 * n + rec_words) + r) * want[1] < 256


def test_planner_refusals():
    assert _plan(20000, 20000, 80000, 1)[0] == UNSUPPORTED          # forced on-chip, nothing fits
    assert _plan(72, 72, 288, 3)[0] == INVALID and _plan(-1, 72, 288)[0] == INVALID and _plan(72, 72, -1)[0] == INVALID
    assert _plan(72, 1 << 28, 0)[0] == INVALID
    L = ldpc._capi.lib()
    assert L.ldpc_debug_stab_tile_plan(72, 72, 288, 0, None, None, None) == 0   # every out pointer may be NULL


# ---- symbols ------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("ldpc_stab_minsum_create", "ldpc_stab_minsum_destroy", "ldpc_stab_minsum_kernel", "ldpc_stab_minsum_tile_syndromes",
               "ldpc_stab_minsum_last_grid", "ldpc_stab_minsum_decode_batch", "ldpc_stab_minsum_decode_batch_device")


def _prototypes(header):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(ldpc_\w+)\s*\(", txt)


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_declared_exported_and_bound(experiments):
    """The entries and THE RULE are in include/ldpc_mi355x_stab.h, the hook in ldpc_mi355x_stab_debug.h, parts of the two
    main headers; both builds export them; no ABI version change."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert tuple(_prototypes("ldpc_mi355x_stab.h")) == NEW_SYMBOLS == ldpc._capi.STAB_SYMBOLS == tuple(ldpc._capi.STAB_API)
    assert tuple(_prototypes("ldpc_mi355x_stab_debug.h")) == ("ldpc_debug_stab_tile_plan",) == ldpc._capi.STAB_DEBUG_SYMBOLS
    assert ldpc._capi.STAB_DEBUG_SYMBOLS == tuple(ldpc._capi.STAB_DEBUG_API)
    hdr, dbg, part = (open(os.path.join(root, "include", f)).read() for f in ("ldpc_mi355x.h", "ldpc_mi355x_debug.h", "ldpc_mi355x_stab.h"))
    assert '#include "ldpc_mi355x_stab.h"' in hdr and '#include "ldpc_mi355x_stab_debug.h"' in dbg
    assert "THE RULE" in part and "typedef struct ldpc_stab_minsum_options" in part and "Consequence." in part
    lib = ldpc._capi.lib(experiments)
    for name in NEW_SYMBOLS + ("ldpc_debug_stab_tile_plan",):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int32, name
    assert lib.ldpc_abi_version() == 4
    assert ctypes.sizeof(ldpc._capi.StabMinSumOptions) == 64
    assert [f[0] for f in ldpc._capi.StabMinSumOptions._fields_] == [f[0] for f in ldpc._capi.PauliMinSumOptions._fields_]
    assert ldpc.StabilizerMinSumDecoder is ldpc.stabilizer.StabilizerMinSumDecoder and callable(ldpc.run_stabilizer_trials)


# ---- ldpc_stab_minsum_create validates before it looks for a device ---------------------------------------------------------

def _pattern(rows, colptr, rowval, keep):
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    keep += [colptr, rowval]
    pat = ldpc._capi.CSSPattern()
    pat.rows, pat.nnz, pat.colptr, pat.rowval = rows, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data
    return pat


# n = 4, r = 2: the stabilizers X X Z Z and Z Z X X
GOOD = dict(n=4, sx=(2, [0, 1, 2, 3, 4], [0, 0, 1, 1]), sz=(2, [0, 1, 2, 3, 4], [1, 1, 0, 0]),
            px=[3.0, 3.0, 3.0, 3.0], py=[3.5, 3.0, 3.0, -1.0], pz=[3.0, 2.0, 3.0, 3.0])


def _create(n, sx, sz, px, py, pz, max_iters=10, alpha=None, clip=None, variant=0, opts=True):
    L = ldpc._capi.lib()
    keep = []
    pats = [ctypes.byref(_pattern(*h, keep)) if h is not None else None for h in (sx, sz)]
    tables = [np.asarray(t, dtype=np.float32) if t is not None else None for t in (px, py, pz)]
    o = ldpc._capi.StabMinSumOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    o.kernel_variant = variant
    h = ctypes.c_void_p()
    st = L.ldpc_stab_minsum_create(n, pats[0], pats[1], *(t.ctypes.data if t is not None else None for t in tables), max_iters,
                                   ctypes.byref(o) if opts else None, ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_stab_minsum_kernel(h) in (1, 2) and L.ldpc_stab_minsum_last_grid(h) == 0
        L.ldpc_stab_minsum_destroy(h)
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
    (dict(sx=None), "sx_part"),
    (dict(sz=None), "sz_part"),
    (dict(sz=(1, [0, 1, 2, 3, 4], [0, 0, 0, 0])), "same number of rows"),                                   # r differs
    (dict(sx=(3, [0, 1, 2, 3, 4], [0, 0, 1, 2])), "same number of rows"),
    (dict(sx=(0, [0, 0, 0, 0, 0], []), sz=(0, [0, 0, 0, 0, 0], [])), "at least one row"),               # r < 1
    (dict(sz=(2, [0, 2, 2, 3, 4], [1, 0, 1, 1])), "ascending"),      # unsorted CSC in the Z part
    (dict(sz=(2, [0, 2, 2, 3, 4], [1, 0, 1, 1])), "sz_part"),
    (dict(sx=(2, [0, 1, 2, 3, 4], [0, 0, 2, 0])), "sx_part"),        # a row out of range in the X part
    (dict(sz=(2, [0, 1, 2, 3, 3], [0, 0, 1, 1])), "sz_part"),        # colptr[n] != nnz
    (dict(n=-1), "n"),
])
def test_create_rejects_bad_arguments_before_any_device_work(change, word):
    st, msg = _create(**{**GOOD, **change})
    assert st == INVALID and word in msg, (st, msg)


def test_create_defaults_and_null_handles():
    """A zeroed options struct means defaults: validation passes, and what answers then is the device lookup -- LDPC_OK
    with a GPU, LDPC_ERR_NO_DEVICE without.  Overlapping patterns (Y-type edges) and one empty pattern pass as well."""
    for kw in (dict(), dict(alpha=0.0, clip=0.0), dict(opts=False), dict(max_iters=0), dict(sz=GOOD["sx"]),
               dict(sz=(2, [0, 0, 0, 0, 0], []))):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (0, NO_DEVICE), (st, msg)
    L = ldpc._capi.lib()
    assert L.ldpc_stab_minsum_kernel(None) == 0 and L.ldpc_stab_minsum_tile_syndromes(None) == 0
    assert L.ldpc_stab_minsum_last_grid(None) == 0 and L.ldpc_stab_minsum_destroy(None) == 0
    assert L.ldpc_stab_minsum_decode_batch(None, 1, None, None, None, None, None, None) == INVALID
    assert L.ldpc_stab_minsum_decode_batch_device(None, 1, None, None, None, None, None, None, None) == INVALID
    assert L.ldpc_stab_minsum_decode_batch_device(None, 0, None, None, None, None, None, None, None) == INVALID
    h = ctypes.c_void_p(1)
    assert L.ldpc_stab_minsum_create(4, None, None, None, None, None, 1, None, None) == INVALID   # out is NULL
    assert L.ldpc_stab_minsum_create(4, None, None, None, None, None, 1, None, ctypes.byref(h)) == INVALID and not h.value


def test_constructor_refusals():
    Sx, Sz = codes.paulis_to_symplectic(["XXZZ", "ZZXX"])
    D = ldpc.StabilizerMinSumDecoder
    for kw in (dict(p=None), dict(p=0.03, pauli_probs=np.full((4, 3), 0.01))):
        with pytest.raises(TypeError):
            D(Sx, Sz, kw.pop("p"), 10, **kw)
    with pytest.raises(TypeError):
        D(Sx, Sz, 0.03, 10.0)
    for probs in ([[0.0, 0.1, 0.1]] * 4, [[0.4, 0.3, 0.3]] * 4, [[0.1, float("nan"), 0.1]] * 4, [[0.1, 0.1, 0.1]] * 3, [[0.1, 0.1]] * 4):
        with pytest.raises(ValueError):
            D(Sx, Sz, None, 10, pauli_probs=probs)
    for p in (0.0, 1.5, (0.5, 0.5, 0.1), (0.0, 0.1, 0.1)):
        with pytest.raises(ValueError):
            D(Sx, Sz, p, 10)
    with pytest.raises(AssertionError, match="do not commute"):
        D.from_paulis(["XXZZ", "ZIII"], 0.03, 10)                        # X and Z meet on one qubit
    with pytest.raises(AssertionError, match="do not commute"):
        D.from_paulis(["XZZXI", "IYIII"], 0.03, 10)                      # Z and Y meet on one qubit
    with pytest.raises(AssertionError):
        D(Sx, Sz[:1], 0.03, 10)                                          # other number of stabilizers
    with pytest.raises(AssertionError):
        D(Sx, Sz[:, :3], 0.03, 10)                                       # other number of qubits
    with pytest.raises(ValueError):
        D.from_paulis(["XZ", "ZXA"], 0.03, 10)
    for kw in (dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")), dict(kernel_variant=3)):
        with pytest.raises(ldpc.LdpcError) as e:
            D(Sx, Sz, 0.03, 10, **kw)
        assert e.value.status == INVALID and e.value.message
    # check=False hands non-commuting rows to the library, which does not look: what answers is the device lookup
    try:
        D.from_paulis(["XXZZ", "ZIII"], 0.03, 10, check=False).close()
    except ldpc.LdpcError as e:
        assert e.status == NO_DEVICE


# ---- codes -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bb72():
    Hx, Hz = codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx) != 0), sp.csc_matrix(np.asarray(Hz) != 0)


@functools.lru_cache(maxsize=None)
def deformed_bb72():
    """BB-72 under `default_rng(7).integers(0, 6, 72)`: 144 X-type, 150 Z-type and 138 Y-type edges."""
    Hx, Hz = bb72()
    Sx, Sz = codes.clifford_deform(Hx, Hz, np.random.default_rng(7).integers(0, 6, 72))
    LSx, LSz = codes.stabilizer_logicals(Sx, Sz)
    return Sx, Sz, LSx, LSz


def _edge_types(Sx, Sz):
    A, B = codes._dense_bits(Sx), codes._dense_bits(Sz)
    return int((A & ~B & 1).sum()), int((B & ~A & 1).sum()), int((A & B).sum())


def test_paulis_and_the_five_qubit_code():
    Sx, Sz = codes.paulis_to_symplectic(["XYZI"])
    assert Sx.tolist() == [[1, 1, 0, 0]] and Sz.tolist() == [[0, 1, 1, 0]] and Sx.dtype == np.uint8
    Fx, Fz = codes.five_qubit_code()
    assert np.array_equal(Fx, codes.paulis_to_symplectic(["XZZXI", "IXZZX", "XIXZZ", "ZXIXZ"])[0])
    assert np.array_equal(Fz, codes.paulis_to_symplectic(["XZZXI", "IXZZX", "XIXZZ", "ZXIXZ"])[1])
    assert not codes.symplectic_product(Fx, Fz, Fx, Fz).any() and _edge_types(Fx, Fz) == (8, 8, 0)
    assert codes.symplectic_product(*codes.paulis_to_symplectic(["X", "Y", "Z"]) * 2).tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]


def test_clifford_deform():
    Hx, Hz = bb72()
    Sx, Sz = codes.clifford_deform(Hx, Hz, np.zeros(72, dtype=np.int64))     # the identity: [Hx; 0], [0; Hz]
    assert np.array_equal(Sx.toarray(), np.vstack([Hx.toarray(), np.zeros((36, 72))]))
    assert np.array_equal(Sz.toarray(), np.vstack([np.zeros((36, 72)), Hz.toarray()]))
    Sx, Sz, _, _ = deformed_bb72()
    assert Sx.shape == Sz.shape == (72, 72) and _edge_types(Sx, Sz) == (144, 150, 138)
    assert np.array_equal(((Sx + Sz) != 0).toarray(), np.vstack([Hx.toarray(), Hz.toarray()]))   # the graph is the CSS code's
    assert not codes.symplectic_product(Sx, Sz, Sx, Sz).any()                # a deformed code commutes
    # every one of the six permutations, on one X-check and one Z-check of one qubit
    for k, perm in enumerate(codes.PAULI_PERMUTATIONS):
        Dx, Dz = codes.clifford_deform([[1]], [[1]], [k])
        letters = ["IXZY"[int(Dx[i, 0]) + 2 * int(Dz[i, 0])] for i in range(2)]
        assert letters == [perm[0], perm[2]]
    with pytest.raises(ValueError):
        codes.clifford_deform(Hx, Hz, np.full(72, 6))
    H = codes.parity_check_csc(12, 4, 3)
    Gx, Gz = codes.hypergraph_product(H, H)
    Dx, Dz = codes.clifford_deform(Gx, Gz, np.random.default_rng(11).integers(0, 6, 225))
    assert Dx.shape == (216, 225) and not codes.symplectic_product(Dx, Dz, Dx, Dz).any() and min(_edge_types(Dx, Dz)) > 100


def test_xzzx_surface_code():
    Sx, Sz = codes.xzzx_surface_code(5)
    assert Sx.shape == Sz.shape == (40, 41) and _edge_types(Sx, Sz)[2] == 0               # no Y-type edge
    weights = np.asarray((Sx + Sz).sum(axis=1)).ravel()
    assert set(weights.tolist()) == {3, 4}
    mixed = (np.asarray(Sx.sum(axis=1)).ravel() > 0) & (np.asarray(Sz.sum(axis=1)).ravel() > 0)
    assert mixed.all()                                                                    # every stabilizer mixes X and Z
    assert not codes.symplectic_product(Sx, Sz, Sx, Sz).any()
    LSx, LSz = codes.stabilizer_logicals(Sx, Sz)
    assert LSx.shape == (2, 41)


@pytest.mark.parametrize("name, k", [("five", 1), ("bb72", 12)])
def test_stabilizer_logicals(name, k):
    if name == "five":
        Sx, Sz = codes.five_qubit_code()
        LSx, LSz = codes.stabilizer_logicals(Sx, Sz)
    else:
        Sx, Sz, LSx, LSz = deformed_bb72()
    n = Sx.shape[1]
    assert LSx.shape == LSz.shape == (2 * k, n) and LSx.dtype == np.uint8
    assert not codes.symplectic_product(Sx, Sz, LSx, LSz).any()                           # commute with every stabilizer
    S = np.concatenate([codes._dense_bits(Sx), codes._dense_bits(Sz)], axis=1)
    L = np.concatenate([LSx, LSz], axis=1)
    assert codes.gf2_rank(np.concatenate([S, L])) == codes.gf2_rank(S) + 2 * k == n + k   # independent modulo the stabilizers
    pairing = np.zeros((2 * k, 2 * k), dtype=np.uint8)
    pairing[np.arange(k), k + np.arange(k)] = pairing[k + np.arange(k), np.arange(k)] = 1
    assert np.array_equal(codes.symplectic_product(LSx, LSz, LSx, LSz), pairing)          # row a anticommutes with row k + a only
    with pytest.raises(AssertionError):
        codes.stabilizer_logicals(*codes.paulis_to_symplectic(["XI", "ZI"]))


# ---- the model ----------------------------------------------------------------------------------------------------------

def test_model_hand_checked_case_with_a_y_type_edge():
    """One stabilizer X Y on two qubits (Sx = [1 1], Sz = [0 1]: an X-type and a Y-type edge), priors 2 (qubit 0) and 1
    (qubit 1) in all three tables, alpha 0.5, s = 1.
    Check sweep 1, all totals +0 so every G is the prior: the X-type edge has u = min(GY, GZ) = 2, w = +0, b = 2; the
    Y-type edge has u = min(GX, GZ) = 1, w = +0, b = 1; m1 = 1 at a = 1, m2 = 2, par = 1: c = (-0.5, -1).
    Bit sweep 1: qubit 0 has MX = -0.5: GX = (2 + 0) + 0 = 2, GY = (2 + 0) - 0.5 = 1.5, GZ = (2 - 0.5) + 0 = 1.5: I (the
    least, 1.5, is > 0).  Qubit 1 has MY = -1: GX = (1 + 0) - 1 = 0, GY = (1 + 0) + 0 = 1, GZ = (1 + 0) - 1 = 0: X and Z
    both anticommute with Y and tie at 0; best starts at X and GZ < GX is false, so X (0 <= 0).  ex = (0, 1), ez = (0, 0):
    the Y-type edge sees ex ^ ez = 1 = s: converged after 1."""
    pr = np.array([2.0, 1.0], dtype=np.float32)
    m = StabMinSumModel([[1, 1]], [[0, 1]], (pr, pr, pr), 5, alpha=0.5)
    gx, gz, conv, its, G = m.decode([[1]])
    assert gx.tolist() == [[0, 1]] and gz.tolist() == [[0, 0]] and conv[0] == 1 and its[0] == 1
    assert G.tolist() == [[[2.0, 0.0], [1.5, 1.0], [1.5, 0.0]]]
    # s = 0: par = 0, c = (0.5, 1): GX = (2, 2), GY = (2.5, 1), GZ = (2.5, 2): nothing to correct
    gx, gz, conv, its, G = m.decode([[0]])
    assert not gx.any() and not gz.any() and conv[0] == 1 and its[0] == 1 and G.tolist() == [[[2.0, 2.0], [2.5, 1.0], [2.5, 2.0]]]
    # a Z-biased qubit 1 (prior_z = 0.5 there) breaks the tie the other way: GZ = (0.5 + 0) - 1 = -0.5 < GX = 0
    gx, gz, conv, its, G = StabMinSumModel([[1, 1]], [[0, 1]], (pr, pr, np.array([2.0, 0.5], dtype=np.float32)), 5, alpha=0.5).decode([[1]])
    assert gx.tolist() == [[0, 0]] and gz.tolist() == [[0, 1]] and conv[0] == 1 and G[0, :, 1].tolist() == [0.0, 1.0, -0.5]


P, TRIALS, ITERS, SEED = 0.06, 400, 30, 0


@functools.lru_cache(maxsize=None)
def statistical_case():
    """The deformed BB-72, depolarizing 0.06, the 400 trials of css_trials_model's sampler at seed 0, 30 iterations: the
    joint model, and the binary min-sum model on [Sz | Sx] (the bits are ex then ez) at the marginal rate 2 p / 3, each
    scored by the binary score over [Sz | Sx] with the logical rows [LSz | LSx].  Computed once, never written to."""
    Sx, Sz, LSx, LSz = deformed_bb72()
    ex, ez = cm.sample(72, TRIALS, P, seed=SEED)
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    joint = StabMinSumModel(Sx, Sz, depolarizing_priors(72, P), ITERS).decode(s)
    H2, L2 = sp.csr_matrix(sp.hstack([Sz, Sx])), np.concatenate([LSz, LSx], axis=1)
    binary = MinSumModel(H2, llr_of_probs(np.full(144, 2.0 * P / 3.0)), ITERS).decode(s)
    e2 = np.concatenate([ex, ez], axis=1)
    _, joint_counts = tm.score(H2, L2, np.concatenate([joint[0], joint[1]], axis=1), e2)
    _, binary_counts = tm.score(H2, L2, binary[0], e2)
    for x in joint + tuple(binary[:2]) + (s, ex, ez):
        x.setflags(write=False)
    assert 0 < joint[2].sum() < TRIALS and len(set(joint[3].tolist())) > 3     # equality tests on this batch are not vacuous
    return dict(s=s, ex=ex, ez=ez, joint=joint, binary=binary, joint_counts=joint_counts, binary_counts=binary_counts)


def test_joint_model_fails_less_often_than_binary_min_sum_on_the_symplectic_matrix():
    """Measured with these models (README): 26 trials with a logical failure and 391 converged under the joint
    rule, against 80 with 356 converged for binary min-sum on [Sz | Sx]."""
    c = statistical_case()
    joint_conv, binary_conv = int(c["joint"][2].sum()), int(c["binary"][1].sum())
    print(f"joint: counts {c['joint_counts'].tolist()} converged {joint_conv}; binary: counts {c['binary_counts'].tolist()} converged {binary_conv}")
    assert c["joint_counts"][0] == c["binary_counts"][0] == TRIALS
    assert c["joint_counts"][3] < c["binary_counts"][3]
    # the measured values the documents quote
    assert c["joint_counts"].tolist() == [400, 28, 9, 26] and joint_conv == 391
    assert c["binary_counts"].tolist() == [400, 89, 44, 80] and binary_conv == 356


def test_model_converged_column_reproduces_the_syndrome():
    c = statistical_case()
    Sx, Sz, _, _ = deformed_bb72()
    gx, gz, conv, its, G = c["joint"]
    ok = conv != 0
    back = symplectic_syndromes(Sx, Sz, gx, gz)
    assert np.array_equal(back[ok], c["s"][ok]) and (back[~ok] != c["s"][~ok]).any(axis=1).all()
    assert (its[~ok] == ITERS).all() and (its[ok] >= 1).all()
    ex, ez = PauliMinSumModel._decide(G[:, 0], G[:, 1], G[:, 2])      # the outputs are the decision on the returned beliefs
    assert np.array_equal(ex, gx != 0) and np.array_equal(ez, gz != 0) and G.dtype == np.float32


def test_model_max_iters_zero():
    Sx, Sz, _, _ = deformed_bb72()
    out = StabMinSumModel(Sx, Sz, depolarizing_priors(72, P), 0).decode(np.ones((3, 72), np.uint8))
    assert all(not x.any() for x in out) and out[4].shape == (3, 3, 72) and out[4].dtype == np.float32 and out[3].dtype == np.int32


def test_model_frozen_column_does_not_change_when_max_iters_grows():
    c = statistical_case()
    Sx, Sz, _, _ = deformed_bb72()
    gx, gz, conv, its, G = c["joint"]
    short = StabMinSumModel(Sx, Sz, depolarizing_priors(72, P), 5).decode(c["s"])
    early = (conv != 0) & (its <= 5)
    assert 0 < early.sum() < TRIALS
    assert np.array_equal(short[2] != 0, early) and np.array_equal(short[3][early], its[early]) and (short[3][~early] == 5).all()
    assert np.array_equal(short[0][early], gx[early]) and np.array_equal(short[1][early], gz[early])
    assert np.array_equal(short[4][early].view(np.int32), G[early].view(np.int32))
    assert (short[4][~early].view(np.int32) != G[~early].view(np.int32)).any()      # the others went on
    one = StabMinSumModel(Sx, Sz, depolarizing_priors(72, P), ITERS).decode(c["s"][7:8])   # a column does not depend on its neighbours
    assert np.array_equal(one[4][0].view(np.int32), G[7].view(np.int32)) and one[3][0] == its[7]


def test_model_on_a_css_input_equals_the_pauli_model_in_every_bit():
    """The consequence the header states: Hx rows as X-type edges, then Hz rows as Z-type edges, s = [sx | sz].  BB-72, 200
    trials at depolarizing 0.06, and once more with per-qubit priors some of which are negative."""
    Hx, Hz = bb72()
    Sx, Sz = codes.clifford_deform(Hx, Hz, np.zeros(72, dtype=np.int64))
    ex, ez = cm.sample(72, 200, P, seed=SEED)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    s = np.concatenate([sx, sz], axis=1)
    assert np.array_equal(s, symplectic_syndromes(Sx, Sz, ex, ez))
    probs = np.random.default_rng(21).uniform(0.002, 0.08, (72, 3))
    probs[[3, 40]], probs[[17, 55]], probs[[29, 71]] = [0.5, 0.1, 0.1], [0.1, 0.55, 0.05], [0.05, 0.1, 0.6]
    from pauli_model import pauli_priors

    for priors, alpha in ((depolarizing_priors(72, P), 0.75), (depolarizing_priors(72, P), 1.0), (pauli_priors(probs), 0.75)):
        a = StabMinSumModel(Sx, Sz, priors, ITERS, alpha=alpha).decode(s)
        b = PauliMinSumModel(Hx, Hz, priors, ITERS, alpha=alpha).decode(sx, sz)
        assert 0 < b[2].sum() < 200 and len(set(b[3].tolist())) > 3
        for x, y in zip(a[:4], b[:4]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert np.array_equal(a[4].view(np.int32), b[4].view(np.int32))          # the LLR planes as bit patterns, -0 included


@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_model_five_qubit_code_all_16_syndromes(alpha):
    """Depolarizing 0.03, 10 iterations, syndrome k = the bits of k (stabilizer i = bit i).  What this model gives:
    alpha 0.75: syndromes 0 .. 14 converge (within 3 iterations), each to a correction of weight <= 1 (the code is perfect:
    the 15 single-qubit Paulis have the 15 nonzero syndromes); syndrome 15 (a Y on qubit 4 would do) runs all 10
    iterations.  alpha 1.0: the 9 syndromes 0, 1, 2, 4, 7, 8, 11, 13, 14 converge in 1 iteration, the other 7 run all 10."""
    Fx, Fz = codes.five_qubit_code()
    syn = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    gx, gz, conv, its, G = StabMinSumModel(Fx, Fz, depolarizing_priors(5, 0.03), 10, alpha=alpha).decode(syn)
    ok = np.nonzero(conv)[0].tolist()
    weight = (gx | gz).sum(axis=1)
    assert np.array_equal(symplectic_syndromes(Fx, Fz, gx, gz)[conv != 0], syn[conv != 0])
    if alpha == 0.75:
        assert ok == list(range(15)) and (weight[:15] <= 1).all() and weight[0] == 0 and (weight[1:15] == 1).all()
        assert its.tolist() == [1, 2, 2, 1, 2, 1, 1, 3, 2, 1, 1, 3, 1, 3, 3, 10]
        assert len({(int(np.argmax(gx[k] | gz[k])), int(gx[k].any()), int(gz[k].any())) for k in range(1, 15)}) == 14   # 14 different Paulis
    else:
        assert ok == [0, 1, 2, 4, 7, 8, 11, 13, 14] and (its[conv != 0] == 1).all() and (its[conv == 0] == 10).all()
        assert weight.tolist() == [0, 1, 1, 3, 1, 3, 3, 5, 1, 3, 3, 5, 3, 5, 5, 0]     # (converged ones of weight 5 among them)


# ---- the table of tests/test_gpu_stab_widths.py -------------------------------------------------------------------------------
# The core is the hypergraph product of two 3-bit repetition checks (n = 13, 6 + 6 checks) under the single-qubit Cliffords of
# default_rng(0).integers(0, 6, 13): 12 checks of union degree 3 or 4, so 48 record words.  Padded with isolated qubits up to n
# and with `empty` empty checks a lane takes 4 (3 n + 48) + 12 + empty = 12 n + 204 + empty bytes.
# n -> (empty, lane bytes, tier, S, the budget S was found under)
KIB79, KIB159 = 79 * 1024, 159 * 1024
STAB_WIDTH_TABLE = {
    80: (4, 1168, 1, 64, KIB79),
    160: (4, 2128, 1, 32, KIB79),
    320: (4, 4048, 1, 16, KIB79),
    640: (4, 7888, 1, 8, KIB79),
    1280: (4, 15568, 1, 4, KIB79),
    2560: (4, 30928, 1, 2, KIB79),
    5120: (4, 61648, 1, 1, KIB79),
    6725: (4, 80908, 1, 2, KIB159),      # one lane misses 79 KiB by 12 bytes; two lanes, 161816 -> 162048, fit 159 KiB: S = 2, not 1
    13550: (12, 162816, 1, 1, KIB159),   # 159 KiB exactly: the largest state that launches on chip
    13600: (4, 163408, 2, 64, 0),        # the unlimited tier by size
}
STAB_WIDTH_REC_WORDS = 48


@functools.lru_cache(maxsize=None)
def stab_width_core():
    """-> (Sx, Sz) 12 x 13 csc: 19 X-, 9 Z- and 12 Y-type edges, union degrees [3, 4, 3, 3, 4, 3, 3, 3, 4, 4, 3, 3]."""
    rep = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    Hx, Hz = codes.hypergraph_product(rep, rep)
    assert Hx.shape == Hz.shape == (6, 13)
    Sx, Sz = codes.clifford_deform(Hx, Hz, np.random.default_rng(0).integers(0, 6, 13))
    assert Sx.shape == Sz.shape == (12, 13) and _edge_types(Sx, Sz) == (19, 9, 12)
    union = np.asarray(((Sx + Sz) != 0).sum(axis=1)).ravel().tolist()
    assert union == [3, 4, 3, 3, 4, 3, 3, 3, 4, 4, 3, 3]
    assert 4 * len(union) == STAB_WIDTH_REC_WORDS                  # every record has the four-word form (degree <= 32)
    return Sx, Sz


def stab_lib_plan(r, n, rec_words, variant=0, experiments=False):
    """(tier, S, state bytes) of the library's plan, or its status where it refuses."""
    L = ldpc._capi.lib(experiments)
    tier, S, state = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    st = L.ldpc_debug_stab_tile_plan(r, n, rec_words, variant, ctypes.byref(tier), ctypes.byref(S), ctypes.byref(state))
    return (tier.value, S.value, state.value) if st == 0 else st


def stab_lane_bytes(r, n, rec_words):
    """One syndrome: MX, MY, MZ (3 n words), the records, the syndrome (bytes)."""
    return 4 * (3 * n + rec_words) + r


def stab_state_bytes(r, n, rec_words, S):
    return (S * stab_lane_bytes(r, n, rec_words) + 255) // 256 * 256


@pytest.mark.parametrize("experiments", [False, True])
@pytest.mark.parametrize("n", sorted(STAB_WIDTH_TABLE))
def test_the_table_of_the_width_tests(n, experiments):
    empty, lane, tier, S, budget = STAB_WIDTH_TABLE[n]
    stab_width_core()
    r, rec = 12 + empty, STAB_WIDTH_REC_WORDS
    bytes_of = lambda w: stab_state_bytes(r, n, rec, w)   # noqa: E731
    assert stab_lane_bytes(r, n, rec) == lane == 12 * n + 204 + empty
    assert stab_lib_plan(r, n, rec, 0, experiments) == (tier, S, bytes_of(S))
    if tier == 1:
        assert stab_lib_plan(r, n, rec, 1, experiments) == (tier, S, bytes_of(S))
        assert bytes_of(S) <= budget and (S == 64 or bytes_of(2 * S) > budget)      # the next wider S misses the budget
        assert (budget == KIB79) == (bytes_of(1) <= KIB79)                          # 159 KiB is tried only where 79 KiB holds nothing
    else:
        assert bytes_of(1) > KIB159 and stab_lib_plan(r, n, rec, 1, experiments) == UNSUPPORTED
    assert stab_lib_plan(r, n, rec, 2, experiments) == (2, 64, bytes_of(64))
    if n == 6725:      # the window: one lane lies in (79 KiB, 159 KiB / 2]
        assert KIB79 + 12 == 80908 <= KIB159 // 2 and 2 * 80908 == 161816 and bytes_of(2) == 162048 <= KIB159
    if n == 13550:     # one more empty check and nothing fits
        assert bytes_of(1) == KIB159 == 162816
        assert stab_lane_bytes(r + 1, n, rec) == 162817 and stab_lib_plan(r + 1, n, rec, 0, experiments)[:2] == (2, 64)
        assert stab_lib_plan(r + 1, n, rec, 1, experiments) == UNSUPPORTED
