"""Per-bit sampling rates and detector error models without a GPU: the model of the per-bit rule (tests/dem_model.py,
the yardstick of tests/test_gpu_dem_trials.py) against the uniform model and against the rule written out, its
statistics, the text form of a detector error model, the phenomenological model against a brute-force simulation, and
the refusals that need no device."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
import dem_model as dm
import trials_model as tm
from ldpcdecoders_jl_amd.dem import DetectorErrorModel, phenomenological, run_dem_trials

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ("ldpc_trials_set_rates", "ldpc_trials_sample_rates_device", "ldpc_trials_sample_rates")
REPETITION = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [0.0, 0.02, 0.5, 1.0])
def test_equal_rates_give_the_uniform_sample_in_every_element(per):
    n, B, seed, c0 = 131, 9, 11, (1 << 40) + 3
    assert np.array_equal(dm.sample(np.full(n, per), B, seed, c0), tm.sample(n, B, per, seed, c0))


def test_the_model_is_the_rule_element_by_element():
    """The vectorised sampler against the rule written out with Python ints."""
    rates = np.array([0.0, 1.0, 2.0 ** -60, 1e-3, 0.25, 1.0 - 2.0 ** -53, 0.5] * 5)
    B, seed, c0 = 6, 5, 1 << 40
    e = dm.sample(rates, B, seed, c0)
    for i in range(B):
        k = tm.mix(seed + tm.GOLDEN * (c0 + i + 1))
        for j, r in enumerate(rates):
            want = 1 if r >= 1.0 else int(tm.mix(k + j) < int(float(r) * 18446744073709551616.0))
            assert e[i, j] == want, (i, j)


def test_thresholds_and_the_free_all_ones_word():
    assert int(dm.thresholds([1.0 - 2.0 ** -53])[0]) == (1 << 64) - (1 << 11)   # the largest threshold of a rate below 1
    assert int(dm.thresholds([2.0 ** -60])[0]) == 16 and int(dm.thresholds([0.5])[0]) == 1 << 63
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dm.sample([0.1, bad], 2)


def test_every_bits_frequency_lies_within_four_and_a_half_standard_deviations():
    """64 bits at rates 0, 1e-4, 0.01, 0.3, 0.5 and 1 over 200,000 columns; the rule is stateless, so the outcome of
    seed 2024 is fixed."""
    rates = np.array(([0.0, 1e-4, 0.01, 0.3, 0.5, 1.0] * 11)[:64])
    N, chunk = 200000, 20000
    ones = np.zeros(64, dtype=np.int64)
    for c0 in range(0, N, chunk):
        ones += dm.sample(rates, chunk, seed=2024, column0=c0).sum(axis=0, dtype=np.int64)
    assert not ones[rates == 0.0].any() and (ones[rates == 1.0] == N).all()
    sd = np.sqrt(rates * (1.0 - rates) / N)
    z = np.abs(ones / N - rates)[sd > 0] / sd[sd > 0]
    print("largest deviation in standard deviations:", float(z.max()))
    assert (z <= 4.5).all(), z


# ---- the text form -----------------------------------------------------------------------------------------------------

def _as_set(d):
    """{(detectors, observables, rate)} of a model: equality up to the order of the mechanisms."""
    H, L = sp.csc_matrix(d.H), sp.csc_matrix(d.L)
    return {(tuple(H.indices[H.indptr[j]:H.indptr[j + 1]]), tuple(L.indices[L.indptr[j]:L.indptr[j + 1]]), float(d.rates[j]))
            for j in range(H.shape[1])}


def _read(name):
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        return f.read()


def test_the_repetition_code_fixture_is_its_phenomenological_model():
    d = DetectorErrorModel.from_text(_read("repetition_d3_r3.dem"))
    want = phenomenological(REPETITION, [[1, 0, 0]], 3, 0.01, 0.02)
    assert d.H.shape == (6, 13) and d.L.shape == (1, 13) and d.num_mechanisms == 13
    assert d == want and np.array_equal(d.channel_probs, want.rates)
    assert d.H.toarray()[:, 1].tolist() == [1, 1, 0, 0, 0, 0] and d.L.toarray()[0].tolist() == [1, 0, 0] * 3 + [0] * 4


def test_the_repeat_fixture_is_the_same_model_in_another_order():
    d = DetectorErrorModel.from_text(_read("repetition_d3_r3_repeat.dem"))
    want = DetectorErrorModel.from_text(_read("repetition_d3_r3.dem"))
    assert d.H.shape == want.H.shape and d.L.shape == want.L.shape and d != want
    assert _as_set(d) == _as_set(want) and len(_as_set(d)) == 13
    assert d.H.toarray()[:, 3].tolist() == [1, 0, 1, 0, 0, 0]        # the first measurement error comes fourth here


def test_round_trip_is_exact():
    rng = np.random.default_rng(3)
    A = (rng.random((30, 40)) < 0.1).astype(np.uint8)
    A[np.arange(40) % 30, np.arange(40)] = 1
    H = sp.csc_matrix(A)
    L = sp.csc_matrix((rng.random((4, 40)) < 0.2).astype(np.uint8))
    cols = {(tuple(H[:, j].toarray().ravel()), tuple(L[:, j].toarray().ravel())) for j in range(40)}
    assert len(cols) == 40 and all(any(h) or any(l) for h, l in cols)
    rates = rng.random(40)
    rates[:4] = (0.0, 1.0, 1.0 - 2.0 ** -53, 1e-300)
    d = DetectorErrorModel(H, L, rates)
    back = DetectorErrorModel.from_text(d.to_text())
    assert back == d and np.array_equal(back.rates.view(np.int64), d.rates.view(np.int64))
    # trailing detectors / observables that no mechanism names survive through a declaration
    wide = DetectorErrorModel(sp.vstack([H, sp.csc_matrix((3, 40), dtype=np.uint8)]), sp.vstack([L, sp.csc_matrix((2, 40), dtype=np.uint8)]), rates)
    text = wide.to_text()
    assert "detector D32" in text and "logical_observable L5" in text
    assert DetectorErrorModel.from_text(text) == wide
    empty = DetectorErrorModel(np.zeros((2, 0)), None, [])
    assert DetectorErrorModel.from_text(empty.to_text()) == empty and empty.L.shape == (0, 0)
    with pytest.raises(ValueError):
        DetectorErrorModel(H, L, rates[:-1])
    with pytest.raises(ValueError):
        DetectorErrorModel(H, L, np.where(np.arange(40) == 7, np.nan, rates))


def test_nested_repeat_with_shift_detectors():
    text = """
    error(0.125) D0          # detector 0
    repeat 2 {
        repeat 3 {
            error(0.25) D0 D1
            shift_detectors 1
        }
        error(0.5) D0 L1
        shift_detectors(0.5, 0, 1) 10
    }
    detector D2
    """
    d = DetectorErrorModel.from_text(text)
    pairs = [(0,), (0, 1), (1, 2), (2, 3), (3,), (13, 14), (14, 15), (15, 16), (16,)]
    assert [tuple(c.nonzero()[0]) for c in d.H.toarray().T] == pairs
    assert d.rates.tolist() == [0.125, 0.25, 0.25, 0.25, 0.5, 0.25, 0.25, 0.25, 0.5]
    assert d.H.shape == (29, 9)                                        # `detector D2` after both shifts: 26 + 2
    assert d.L.shape == (2, 9) and d.L.toarray()[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1] and not d.L.toarray()[0].any()


def test_cancel_merge_and_drop_rules():
    d = DetectorErrorModel.from_text("error(0.1) D1 D3 ^ D1 L0 L0 L2\n")
    assert d.H.toarray().ravel().tolist() == [0, 0, 0, 1] and d.L.toarray().ravel().tolist() == [0, 0, 1]
    p1, p2, p3 = 0.1, 0.3, 0.07
    d = DetectorErrorModel.from_text(f"error({p1!r}) D0 D1\nerror(0.5) D2\nerror({p2!r}) D1 ^ D0\nerror({p3!r}) D0 D1 D2 D2\n")
    assert d.H.shape == (3, 2) and d.rates[1] == 0.5
    first = p1 + p2 - 2.0 * p1 * p2
    assert d.rates[0] == first + p3 - 2.0 * first * p3                 # in order of appearance, exactly
    assert DetectorErrorModel.from_text("error(0.25) D0\nerror(0.25) D0\n").rates.tolist() == [0.375]
    # the same detectors with another observable are another effect
    assert DetectorErrorModel.from_text("error(0.25) D0\nerror(0.25) D0 L0\n").num_mechanisms == 2
    # an empty effect is dropped, but what it names still counts
    d = DetectorErrorModel.from_text("error(0.2) D4 D4\nerror(0.3)\nerror(0.4) D1\nerror(0.1) L3 L3\n")
    assert d.H.shape == (5, 1) and d.L.shape == (4, 1) and d.rates.tolist() == [0.4]


@pytest.mark.parametrize("text, line", [
    ("error(0.1) D0\nerror(0.1) X3\n", 2),
    ("error(0.1) D0\n\n# a comment\nerror(1.5) D1\n", 4),
    ("error(nan) D0\n", 1),
    ("error D0\n", 1),
    ("error(0.1, 0.2) D0\n", 1),
    ("error(0.1) D0\nmeasure D0\n", 2),
    ("error(0.1) D0\n}\n", 2),
    ("repeat 2 {\nerror(0.1) D0\n", 1),
    ("error(0.1) D0\nrepeat x {\n}\n", 2),
    ("error(0.1) D0\nrepeat 2\nerror(0.1) D1\n", 2),
    ("shift_detectors D1\n", 1),
    ("error(0.1) D0\nerror(0.2) D-1\n", 2),
    ("error(0.1) D0\n???\n", 2),
])
def test_a_malformed_line_is_named_by_its_number(text, line):
    with pytest.raises(ValueError) as ei:
        DetectorErrorModel.from_text(text)
    assert f"line {line}:" in str(ei.value), str(ei.value)


# ---- the phenomenological model ------------------------------------------------------------------------------------------

def _simulate(H, L, R, e):
    """Brute force, one mechanism vector at a time: data errors accumulate round by round, every round but the last
    reports flipped outcomes, detectors are differences of consecutive rounds, observables see the final data error."""
    s, n = H.shape
    data = e[:R * n].reshape(R, n)
    meas = e[R * n:].reshape(R - 1, s)
    held = np.zeros(n, dtype=np.int64)
    before = np.zeros(s, dtype=np.int64)
    detectors = []
    for t in range(R):
        held = held ^ data[t]
        outcome = (H @ held) % 2
        if t < R - 1:
            outcome = outcome ^ meas[t]
        detectors.append(outcome ^ before)
        before = outcome
    return np.concatenate(detectors), (L @ held) % 2


def _check_against_simulation(H, L, R, seed):
    H = np.asarray(sp.csr_matrix(H).todense()).astype(np.int64)
    L = np.asarray(sp.csr_matrix(L).todense()).astype(np.int64)
    s, n = H.shape
    rng = np.random.default_rng(seed)
    p, q = rng.uniform(0.001, 0.1, size=n), rng.uniform(0.001, 0.1, size=s)
    d = phenomenological(H, L, R, p, q)
    assert d.H.shape == (R * s, R * n + (R - 1) * s) and d.L.shape == (L.shape[0], R * n + (R - 1) * s)
    assert np.array_equal(d.rates, np.concatenate([np.tile(p, R), np.tile(q, R - 1)]))
    Hd, Ld = d.H.toarray().astype(np.int64), d.L.toarray().astype(np.int64)
    E = (rng.random((2000, d.num_mechanisms)) < 0.15).astype(np.int64)
    got_d, got_l = (E @ Hd.T) % 2, (E @ Ld.T) % 2
    assert got_d.any() and (L.shape[0] == 0 or got_l.any())
    for b in range(2000):
        want_d, want_l = _simulate(H, L, R, E[b])
        assert np.array_equal(got_d[b], want_d) and np.array_equal(got_l[b], want_l), b
    return d


@pytest.mark.parametrize("R", [1, 2, 4])
def test_phenomenological_equals_a_brute_force_simulation_on_a_small_code(R):
    H = ldpc.codes.parity_check_csc(24, 6, 3)
    L = (np.random.default_rng(9).random((3, 24)) < 0.3).astype(np.uint8)
    d = _check_against_simulation(H, L, R, seed=R)
    if R == 1:
        assert (d.H != sp.csc_matrix(H)).nnz == 0                       # one perfect round is the code itself


def test_phenomenological_equals_a_brute_force_simulation_on_bb72():
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    d = _check_against_simulation(Hx, Lz, 3, seed=72)
    assert d.H.shape == (108, 288) and d.L.shape == (12, 288)
    scalar = phenomenological(Hx, None, 3, 0.01, 0.02)
    assert scalar.L.shape == (0, 288) and scalar.rates.tolist() == [0.01] * 216 + [0.02] * 72
    with pytest.raises(ValueError):
        phenomenological(Hx, Lz, 0, 0.01, 0.02)


# ---- exports and refusals ------------------------------------------------------------------------------------------------

def test_the_package_exports_the_new_names():
    for name in ("DetectorErrorModel", "phenomenological", "run_dem_trials"):
        assert hasattr(ldpc, name) and name in ldpc.__all__
    for name in ("set_rates", "sample_rates", "sample_rates_host"):
        assert hasattr(ldpc.Trials, name)


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_by_both_builds(experiments):
    lib = ldpc._capi.lib(experiments)
    for name in NEW_SYMBOLS:
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ldpc_abi_version() == 4   # added by symbol


def _stand_in(H):
    """What run_trials reads of a decoder before its first library call."""
    return SimpleNamespace(sparse_H=sp.csc_matrix(H), per=None)


def test_rates_of_the_wrong_length_are_refused_before_any_library_call():
    dec = _stand_in(REPETITION)
    for per in (np.full(2, 0.1), np.full(4, 0.1), np.full((3, 1), 0.1), []):
        with pytest.raises(ValueError) as ei:
            ldpc.run_trials(dec, 10, per=per)
        assert "one rate per bit" in str(ei.value)


def test_run_dem_trials_refuses_a_decoder_of_another_matrix():
    d = phenomenological(REPETITION, [[1, 0, 0]], 3, 0.01, 0.02)
    other = d.H.copy().tolil()
    other[0, 1] = 0
    for H in (REPETITION, other, d.H[:, :-1], d.H[:-1, :]):
        with pytest.raises(ValueError) as ei:
            run_dem_trials(d, _stand_in(H), 10)
        assert "check matrix" in str(ei.value)


def test_argument_validation_happens_before_any_device_work():
    lib = ldpc._capi.lib()
    err = lambda: lib.ldpc_last_error()   # noqa: E731
    rates = np.full(8, 0.1)
    assert lib.ldpc_trials_set_rates(None, 8, rates.ctypes.data) == 1 and b"handle" in err()
    assert lib.ldpc_trials_set_rates(None, 8, None) == 1 and b"handle" in err()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for entry, extra in ((lib.ldpc_trials_sample_rates_device, (None,)), (lib.ldpc_trials_sample_rates, ())):
        assert entry(None, -1, 0, 0, p, p, *extra) == 1 and b"batch" in err()
        assert entry(None, 1, -1, 0, p, p, *extra) == 1 and b"column0" in err()
        assert entry(None, 1, 0, 0, None, p, *extra) == 1 and b"errors" in err()
        assert entry(None, 1, 0, 0, p, None, *extra) == 1 and b"handle" in err()
        assert entry(None, 0, 0, 0, None, None, *extra) == 1 and b"handle" in err()
    assert not buf.any()
    if lib.ldpc_device_count() == 0:
        with pytest.raises(ldpc.LdpcError) as ei:
            phenomenological(REPETITION, None, 2, 0.01, 0.02).trials()
        assert ei.value.status == 2   # LDPC_ERR_NO_DEVICE, no CPU fallback
