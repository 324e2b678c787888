"""CSS-code Monte-Carlo trial steps without a GPU: the model (tests/css_trials_model.py, the yardstick of
tests/test_gpu_css_trials.py) checks itself against the stated rule and against the one-matrix model, the host
elimination finds paired logical operators, the product family commutes, and the new C entries are declared as the
header states them and validate their arguments before any device work."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ldpcdecoders_jl_amd as ldpc
import css_trials_model as cm
import trials_model as tm

css_trials = ldpc.css_trials   # the unit under test: without it this file does not import, its model self-checks included

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldpc_css_trials_create", "ldpc_css_trials_destroy", "ldpc_css_trials_kernel", "ldpc_css_trials_sample_device",
               "ldpc_css_trials_syndromes_device", "ldpc_css_trials_score_device", "ldpc_css_trials_sample", "ldpc_css_trials_score")


def _gf2(A, B):
    return (np.asarray(A).astype(np.int64) @ np.asarray(B).astype(np.int64)) % 2


def _dense(M):
    return np.asarray(M.todense() if hasattr(M, "todense") else M).astype(np.uint8)


# ---- the model ------------------------------------------------------------------------------------------------------
def test_the_model_is_the_rule_element_by_element():
    n, B, seed, c0 = 37, 5, 11, 1 << 40
    px, py, pz = 0.1, 0.05, 0.2
    ex, ez = cm.sample(n, B, (px, py, pz), seed, c0)
    a = int(px * 18446744073709551616.0)
    b = a + int(py * 18446744073709551616.0)
    c = b + int(pz * 18446744073709551616.0)
    for i in range(B):
        k = tm.mix(seed + tm.GOLDEN * (c0 + i + 1))
        for j in range(n):
            r = tm.mix(k + j)
            assert ex[i, j] == (r < b) and ez[i, j] == (a <= r < c)


@pytest.mark.parametrize("px", [0.0, 0.02, 0.5, 1e-12])
def test_x_only_noise_is_the_one_matrix_rule(px):
    """py = pz = 0: ex is trials_model.sample at per = px in every element, ez is zero."""
    for seed, c0 in ((0, 0), (0xDEADBEEFCAFE1234, (1 << 40) + 3)):
        ex, ez = cm.sample(131, 9, (px, 0.0, 0.0), seed, c0)
        assert np.array_equal(ex, tm.sample(131, 9, px, seed, c0))
        assert not ez.any()


def test_column0_rule():
    whole = cm.sample(131, 9, 0.3, seed=5, column0=7)
    for i in range(9):
        one = cm.sample(131, 1, 0.3, seed=5, column0=7 + i)
        assert np.array_equal(whole[0][i], one[0][0]) and np.array_equal(whole[1][i], one[1][0])
    assert not np.array_equal(whole[0], cm.sample(131, 9, 0.3, seed=6, column0=7)[0])


def test_every_qubit_has_exactly_one_pauli():
    P = cm.paulis(200, 50, (0.2, 0.1, 0.3), seed=3)
    ex, ez = cm.sample(200, 50, (0.2, 0.1, 0.3), seed=3)
    kinds = [(P == k) for k in (cm.PAULI_I, cm.PAULI_X, cm.PAULI_Y, cm.PAULI_Z)]
    assert (sum(k.astype(np.int64) for k in kinds) == 1).all() and all(k.any() for k in kinds)
    # (ex, ez) names the Pauli: I = 00, X = 10, Y = 11, Z = 01
    assert np.array_equal(kinds[0], (ex == 0) & (ez == 0)) and np.array_equal(kinds[1], (ex == 1) & (ez == 0))
    assert np.array_equal(kinds[2], (ex == 1) & (ez == 1)) and np.array_equal(kinds[3], (ex == 0) & (ez == 1))


def test_pauli_frequencies_within_four_standard_deviations():
    p, N = 0.03, 4096 * 1000
    P = cm.paulis(1000, 4096, p, seed=0)
    sd = math.sqrt((p / 3) * (1 - p / 3) / N)
    for kind in (cm.PAULI_X, cm.PAULI_Y, cm.PAULI_Z):
        mean = (P == kind).mean(dtype=np.float64)
        assert abs(mean - p / 3) <= 4 * sd, (kind, mean, (mean - p / 3) / sd)


def test_bad_rates_are_rejected():
    for rates in ((0.5, 0.5, 0.0), (0.4, 0.3, 0.4), (float("nan"), 0.0, 0.0), (0.0, -0.1, 0.0), (0.0, 0.0, 1.0), (1.5, 0.0, 0.0)):
        with pytest.raises(ValueError):
            cm.sample(4, 4, rates)
    assert cm.thresholds(0.5, 0.25, 0.125) == (1 << 63, 3 << 62, 7 << 61)
    assert not any(x.any() for x in cm.sample(200, 50, (0.0, 0.0, 0.0)))


def test_syndromes_and_score_of_the_model_on_a_hand_checked_case():
    Hx = np.array([[1, 1, 1, 1]], dtype=np.uint8)
    Hz = np.array([[1, 1, 0, 0], [0, 0, 1, 1]], dtype=np.uint8)      # [[4,1]]: commute
    Lx = np.array([[1, 1, 0, 0]], dtype=np.uint8)
    Lz = np.array([[1, 0, 1, 0]], dtype=np.uint8)
    ex = np.array([[1, 0, 0, 0], [3, 2, 0, 1]], dtype=np.uint8)      # only the low bits count
    ez = np.array([[0, 1, 0, 0], [1, 1, 0, 0]], dtype=np.uint8)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    assert sx.tolist() == [[1], [0]] and sz.tolist() == [[1, 0], [1, 1]]
    z = np.zeros((4, 4), dtype=np.uint8)
    gx = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=np.uint8)
    gz = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 1, 0]], dtype=np.uint8)
    flags, counts = cm.score(Hx, Hz, Lx, Lz, gx, gz, z, z)
    # column 1: dx = 1000 breaks a Z check and anticommutes with Lz; column 2: dx = 1111 is the row of Hx, a stabilizer
    # (bit 0 only); column 3: dz = 1010 = Lz commutes with Hx and anticommutes with Lx: bits 0 and 3
    assert flags.tolist() == [0, 1 | 2 | 4, 1, 1 | 8] and counts.tolist() == [4, 3, 1, 2, 1, 1]
    flags, counts = cm.score(Hx, Hz, None, None, gx, gz, z, z)
    assert flags.tolist() == [0, 3, 1, 1] and counts.tolist() == [4, 3, 1, 0, 0, 0]


# ---- codes ----------------------------------------------------------------------------------------------------------
def _check_logicals(Hx, Hz, k_expected=None, paired=True):
    Hx, Hz = _dense(Hx), _dense(Hz)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    k = Hx.shape[1] - ldpc.codes.gf2_rank(Hx) - ldpc.codes.gf2_rank(Hz)
    if k_expected is not None:
        assert k == k_expected
    assert Lx.shape == (k, Hx.shape[1]) and Lz.shape == (k, Hx.shape[1])
    assert not _gf2(Hz, Lx.T).any() and not _gf2(Hx, Lz.T).any()
    assert ldpc.codes.gf2_rank(np.concatenate([Hx, Lx])) == ldpc.codes.gf2_rank(Hx) + k
    assert ldpc.codes.gf2_rank(np.concatenate([Hz, Lz])) == ldpc.codes.gf2_rank(Hz) + k
    if paired:
        assert np.array_equal(_gf2(Lx, Lz.T), np.eye(k, dtype=np.int64))
    return Lx, Lz


def test_css_logicals_on_bb72():
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    Lx, Lz = _check_logicals(HX, HZ, k_expected=12)
    assert Lx.shape[0] == 12 and Lz.shape[0] == 12


def test_css_logicals_on_a_hypergraph_product():
    Hx, Hz = ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(12, 4, 3))
    _check_logicals(Hx, Hz)


def test_css_logicals_refuses_a_non_commuting_pair():
    with pytest.raises(AssertionError):
        ldpc.codes.css_logicals(np.array([[1, 0]]), np.array([[1, 1]]))


def test_hypergraph_product_shapes_and_commutation():
    H1 = ldpc.parity_check_matrix(12, 4, 3)          # 9 x 12
    H2 = ldpc.parity_check_matrix(10, 5, 2, seed=3)  # 4 x 10
    for A, B in ((H1, None), (H1, H2)):
        Hx, Hz = ldpc.codes.hypergraph_product(A, B)
        Bm = A if B is None else B
        (m1, n1), (m2, n2) = A.shape, Bm.shape
        assert Hx.shape == (m1 * n2, n1 * n2 + m1 * m2) and Hz.shape == (n1 * m2, n1 * n2 + m1 * m2)
        a, b = A.astype(np.int64), Bm.astype(np.int64)
        assert np.array_equal(_dense(Hx), np.concatenate([np.kron(a, np.eye(n2)), np.kron(np.eye(m1), b.T)], axis=1))
        assert np.array_equal(_dense(Hz), np.concatenate([np.kron(np.eye(n1), b), np.kron(a.T, np.eye(m2))], axis=1))
        assert not _gf2(_dense(Hx), _dense(Hz).T).any()
    Hx, Hz = ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(60, 6, 3))
    assert Hx.shape == (1800, 4500) and Hz.shape == (1800, 4500)


# ---- the package and the C boundary ---------------------------------------------------------------------------------
def test_the_package_exports_the_new_names():
    for name in ("CSSTrials", "CSSTrialResult", "run_css_trials"):
        assert hasattr(ldpc, name) and name in ldpc.__all__ and getattr(ldpc, name) is getattr(css_trials, name)
    r = ldpc.CSSTrialResult(trials=200, block_errors=8, syndrome_mismatches=2, logical_errors=5, logical_x_errors=3,
                            logical_z_errors=4, not_converged_hx=1, not_converged_hz=6)
    assert (r.block_error_rate, r.syndrome_mismatch_rate, r.logical_error_rate) == (0.04, 0.01, 0.025)
    assert (r.logical_x_error_rate, r.logical_z_error_rate, r.not_converged_hx_rate, r.not_converged_hz_rate) == (0.015, 0.02, 0.005, 0.03)
    assert "2 p / 3" in ldpc.run_css_trials.__doc__


def test_csstrials_check_refuses_a_non_commuting_pair_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise RuntimeError("the library was reached")

    monkeypatch.setattr(ldpc._capi, "lib_for", no_library)
    with pytest.raises(AssertionError):
        ldpc.CSSTrials(np.array([[1, 0]]), np.array([[1, 1]]), logicals=False)
    with pytest.raises(AssertionError):
        ldpc.CSSTrials(np.array([[1, 1, 0]]), np.array([[1, 1]]), logicals=False)   # unequal n


_CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double,
           "ldpc_status": ctypes.c_int32}


def _prototypes():
    """name -> (return type, [parameter types]) of the ldpc_css_trials_* prototypes of the header; a pointer is '*'."""
    txt = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(\w+)\s+(ldpc_css_trials_\w+)\s*\(([^)]*)\)\s*;", txt):
        kinds = []
        for prm in params.split(","):
            prm = prm.strip()
            kinds.append("*" if ("*" in prm or "[" in prm) else prm.replace("const ", "").split()[0])
        out[name] = (ret, kinds)
    return out


@pytest.mark.parametrize("experiments", [False, True])
def test_capi_declares_the_new_symbols_with_the_headers_signatures(experiments):
    lib = ldpc._capi.lib(experiments)
    protos = _prototypes()
    assert sorted(protos) == sorted(NEW_SYMBOLS)
    for name, (ret, kinds) in protos.items():
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is _CTYPES[ret], name
        assert len(fn.argtypes) == len(kinds), name
        for got, kind in zip(fn.argtypes, kinds):
            if kind == "*":
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, got)
            else:
                assert got is _CTYPES[kind], (name, got, kind)
    assert lib.ldpc_abi_version() == 4   # added by symbol
    assert ctypes.sizeof(ldpc._capi.CSSTrialsOptions) == 64 and ctypes.sizeof(ldpc._capi.CSSPattern) == 32


def _pattern(rows, colptr, rowval):
    pat = ldpc._capi.CSSPattern()
    pat.rows, pat.nnz = rows, len(rowval) if rowval is not None else 0
    pat.colptr = colptr.ctypes.data if colptr is not None else None
    pat.rowval = rowval.ctypes.data if rowval is not None and len(rowval) else None
    return pat


def test_argument_validation_happens_before_any_device_work():
    lib = ldpc._capi.lib()
    err = lambda: lib.ldpc_last_error()   # noqa: E731
    h = ctypes.c_void_p()
    colptr = np.array([0, 2, 2], dtype=np.int64)
    good = np.array([0, 1], dtype=np.int64)
    ok = _pattern(2, colptr, good)
    R = ctypes.byref

    def create(hx, hz, lx=None, lz=None, opts=None, n=2):
        return lib.ldpc_css_trials_create(n, hx, hz, lx, lz, opts, R(h))

    for bad, word in ((np.array([1, 0], dtype=np.int64), b"ascending"), (np.array([0, 5], dtype=np.int64), b"outside")):
        b = _pattern(2, colptr, bad)
        for args, who in (((R(b), R(ok)), b"Hx"), ((R(ok), R(b)), b"Hz"), ((R(ok), R(ok), R(b)), b"Lx"), ((R(ok), R(ok), None, R(b)), b"Lz")):
            assert create(*args) == 1 and who in err() and word in err() and not h.value
    assert create(None, R(ok)) == 1 and b"Hx" in err()
    assert create(R(ok), None) == 1 and b"Hz" in err()
    three = _pattern(2, colptr, good)
    three.nnz = 3
    assert create(R(three), R(ok)) == 1
    assert create(R(ok), R(ok), n=-1) == 1
    neg = _pattern(-1, None, None)
    assert create(R(ok), R(ok), R(neg)) == 1 and b"rows" in err()
    stray = _pattern(0, None, None)
    stray.nnz = 3
    assert create(R(ok), R(ok), None, R(stray)) == 1 and b"nnz" in err()
    nullptrs = _pattern(2, None, None)
    nullptrs.nnz = 2
    assert create(R(ok), R(ok), R(nullptrs)) == 1 and b"colptr" in err()
    assert lib.ldpc_css_trials_create(2, R(ok), R(ok), None, None, None, None) == 1 and b"out" in err()
    o = ldpc._capi.CSSTrialsOptions()
    o.device, o.kernel_variant = -1, 3
    assert create(R(ok), R(ok), opts=R(o)) == 1 and b"kernel_variant" in err()
    # the batch entries: scalars and required pointers, then the handle
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for entry, extra in ((lib.ldpc_css_trials_sample_device, (None,)), (lib.ldpc_css_trials_sample, ())):
        assert entry(None, -1, 0, 0.1, 0.1, 0.1, 0, p, p, p, p, *extra) == 1 and b"batch" in err()
        assert entry(None, 1, -1, 0.1, 0.1, 0.1, 0, p, p, p, p, *extra) == 1 and b"column0" in err()
        for rates in ((-0.1, 0, 0), (0, 1.0, 0), (0, 0, float("nan")), (1.5, 0, 0)):
            assert entry(None, 1, 0, *rates, 0, p, p, p, p, *extra) == 1 and b"[0, 1)" in err()
        for rates in ((0.5, 0.5, 0.0), (0.4, 0.3, 0.4)):
            assert entry(None, 1, 0, *rates, 0, p, p, p, p, *extra) == 1 and b"overflow" in err()
        assert entry(None, 1, 0, 0.1, 0.1, 0.1, 0, None, p, p, p, *extra) == 1 and b"ex" in err()
        assert entry(None, 1, 0, 0.1, 0.1, 0.1, 0, p, None, p, p, *extra) == 1 and b"ez" in err()
        assert entry(None, 1, 0, 0.1, 0.1, 0.1, 0, p, p, None, None, *extra) == 1 and b"handle" in err()
        assert entry(None, 0, 0, 0.1, 0.1, 0.1, 0, None, None, None, None, *extra) == 1 and b"handle" in err()
    synd = lib.ldpc_css_trials_syndromes_device
    assert synd(None, -1, p, p, p, p, None) == 1 and b"batch" in err()
    for k, word in enumerate((b"ex", b"ez", b"sx", b"sz")):
        args = [p, p, p, p]
        args[k] = None
        assert synd(None, 1, *args, None) == 1 and word in err()
    assert synd(None, 1, p, p, p, p, None) == 1 and b"handle" in err()
    for entry, extra in ((lib.ldpc_css_trials_score_device, (None,)), (lib.ldpc_css_trials_score, ())):
        assert entry(None, -1, p, p, p, p, p, p, *extra) == 1 and b"batch" in err()
        for k, word in enumerate((b"gx", b"gz", b"ex", b"ez", None, b"counts")):
            if word is None:
                continue
            args = [p] * 6
            args[k] = None
            assert entry(None, 1, *args, *extra) == 1 and word in err()
        assert entry(None, 1, p, p, p, p, None, p, *extra) == 1 and b"handle" in err()
    assert lib.ldpc_css_trials_destroy(None) == 0 and lib.ldpc_css_trials_kernel(None) == 0
    if lib.ldpc_device_count() == 0:
        assert create(R(ok), R(ok)) == 2 and not h.value   # LDPC_ERR_NO_DEVICE, no CPU fallback
        HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
        with pytest.raises(ldpc.LdpcError) as ei:
            ldpc.CSSTrials(HX, HZ)
        assert ei.value.status == 2
