"""Monte-Carlo trial steps without a GPU: the model (tests/trials_model.py, the yardstick of tests/test_gpu_trials.py)
checks itself against the stated rule, the package exports the new names, and the new C entries validate their
arguments before any device work."""
import ctypes
import math

import numpy as np
import pytest

import ldpcdecoders_jl_amd as ldpc
import bitflip_model
import trials_model as tm

NEW_SYMBOLS = ("ldpc_trials_create", "ldpc_trials_destroy", "ldpc_trials_kernel", "ldpc_trials_sample_device",
               "ldpc_trials_syndromes_device", "ldpc_trials_score_device", "ldpc_trials_sample", "ldpc_trials_score")


def test_mix_is_the_bitflip_models_mix():
    assert tm.GOLDEN == bitflip_model.GOLDEN
    zs = [0, 1, tm.GOLDEN, 2 * tm.GOLDEN, tm.MASK, 0x0123456789ABCDEF, 1 << 63]
    for z in zs:
        assert tm.mix(z) == bitflip_model.mix(z)
    arr = tm.mix_array(np.array([z & tm.MASK for z in zs], dtype=np.uint64))
    assert [int(x) for x in arr] == [bitflip_model.mix(z) for z in zs]


def test_the_model_is_the_rule_element_by_element():
    """The vectorised sampler against the rule written out with Python ints."""
    n, B, per, seed, c0 = 37, 5, 0.3, 11, 1 << 40
    e = tm.sample(n, B, per, seed, c0)
    t = int(per * 18446744073709551616.0)
    for i in range(B):
        k = bitflip_model.mix(seed + tm.GOLDEN * (c0 + i + 1))
        for j in range(n):
            assert e[i, j] == (bitflip_model.mix(k + j) < t)


def test_column0_rule():
    """Column i of a call with column0 = c is column 0 of a call with column0 = c + i; a split call is the whole."""
    whole = tm.sample(131, 9, 0.2, seed=5, column0=7)
    for i in range(9):
        assert np.array_equal(whole[i], tm.sample(131, 1, 0.2, seed=5, column0=7 + i)[0])
    assert np.array_equal(whole, np.concatenate([tm.sample(131, 3, 0.2, 5, 7), tm.sample(131, 6, 0.2, 5, 10)]))
    assert not np.array_equal(whole, tm.sample(131, 9, 0.2, seed=6, column0=7))


def test_thresholds():
    assert tm.threshold(1e-12) == 18446744
    assert tm.threshold(0.0) == 0 and tm.threshold(0.5) == 1 << 63
    assert not tm.sample(200, 50, 0.0).any()
    assert tm.sample(200, 50, 1.0).all()
    with pytest.raises(ValueError):
        tm.sample(4, 4, 1.5)
    with pytest.raises(ValueError):
        tm.sample(4, 4, float("nan"))


@pytest.mark.parametrize("per", [0.01, 0.02, 0.5, 0.001])
def test_overall_mean_within_four_standard_deviations(per):
    N = 4096 * 1000
    mean = tm.sample(1000, 4096, per, seed=0).mean(dtype=np.float64)
    sd = math.sqrt(per * (1 - per) / N)
    assert abs(mean - per) <= 4 * sd, (mean, per, (mean - per) / sd)


def test_syndromes_and_score_of_the_model_on_a_hand_checked_case():
    H = np.array([[1, 1, 0, 0], [0, 1, 1, 0]], dtype=np.uint8)      # kernel: 1110, 0001
    L = np.array([[0, 0, 0, 1]], dtype=np.uint8)
    e = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [3, 2, 0, 0]], dtype=np.uint8)   # only the low bits count
    assert tm.syndromes(H, e).tolist() == [[1, 0], [1, 1], [1, 0]]
    errors = np.zeros((4, 4), dtype=np.uint8)
    guesses = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 1]], dtype=np.uint8)
    flags, counts = tm.score(H, L, guesses, errors)
    assert flags.tolist() == [0, 3, 1, 5] and counts.tolist() == [4, 3, 1, 1]
    flags, counts = tm.score(H, None, guesses, errors)
    assert flags.tolist() == [0, 3, 1, 1] and counts.tolist() == [4, 3, 1, 0]


def test_the_package_exports_the_new_names():
    for name in ("Trials", "TrialResult", "run_trials"):
        assert hasattr(ldpc, name) and name in ldpc.__all__
    r = ldpc.TrialResult(trials=200, block_errors=3, syndrome_mismatches=2, logical_errors=1, not_converged=4)
    assert (r.block_error_rate, r.syndrome_mismatch_rate, r.logical_error_rate, r.not_converged_rate) == (0.015, 0.01, 0.005, 0.02)
    assert hasattr(ldpc.BPOTSDecoder, "decode_batch_device")


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_by_both_builds(experiments):
    lib = ldpc._capi.lib(experiments)
    for name in NEW_SYMBOLS:
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ldpc_abi_version() == 4   # added by symbol
    assert ctypes.sizeof(ldpc._capi.TrialsOptions) == 64


def test_argument_validation_happens_before_any_device_work():
    lib = ldpc._capi.lib()
    err = lambda: lib.ldpc_last_error()   # noqa: E731
    h = ctypes.c_void_p()
    colptr = np.array([0, 2, 2], dtype=np.int64)
    good = np.array([0, 1], dtype=np.int64)
    create = lambda *a: lib.ldpc_trials_create(*a, ctypes.byref(h))   # noqa: E731
    cp, gp = colptr.ctypes.data, good.ctypes.data
    for bad, word in ((np.array([1, 0], dtype=np.int64), b"ascending"), (np.array([0, 5], dtype=np.int64), b"outside")):
        assert create(2, 2, 2, cp, bad.ctypes.data, 0, 0, None, None, None) == 1 and word in err() and not h.value
        # the same checks on the logical rows, which name themselves
        assert create(2, 2, 2, cp, gp, 2, 2, cp, bad.ctypes.data, None) == 1 and b"logical" in err() and word in err()
    assert create(2, 2, 3, cp, gp, 0, 0, None, None, None) == 1
    assert create(2, 2, 2, cp, gp, -1, 0, None, None, None) == 1 and b"nl" in err()
    assert create(2, 2, 2, cp, gp, 0, 3, None, None, None) == 1 and b"lnnz" in err()
    assert create(2, 2, 2, cp, gp, 2, 2, None, None, None) == 1 and b"lcolptr" in err()
    assert lib.ldpc_trials_create(2, 2, 2, cp, gp, 0, 0, None, None, None, None) == 1 and b"out" in err()
    o = ldpc._capi.TrialsOptions()
    o.device, o.kernel_variant = -1, 3
    assert create(2, 2, 2, cp, gp, 0, 0, None, None, ctypes.byref(o)) == 1 and b"kernel_variant" in err()
    # the batch entries: scalars and required pointers, then the handle
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for entry, extra in ((lib.ldpc_trials_sample_device, (None,)), (lib.ldpc_trials_sample, ())):
        assert entry(None, -1, 0, 0.1, 0, p, p, *extra) == 1 and b"batch" in err()
        assert entry(None, 1, -1, 0.1, 0, p, p, *extra) == 1 and b"column0" in err()
        for per in (-0.1, 1.5, float("nan")):
            assert entry(None, 1, 0, per, 0, p, p, *extra) == 1 and b"per" in err()
        assert entry(None, 1, 0, 0.1, 0, None, p, *extra) == 1 and b"errors" in err()
        assert entry(None, 1, 0, 0.1, 0, p, None, *extra) == 1 and b"handle" in err()
    assert lib.ldpc_trials_syndromes_device(None, -1, p, p, None) == 1 and b"batch" in err()
    assert lib.ldpc_trials_syndromes_device(None, 1, None, p, None) == 1 and b"errors" in err()
    assert lib.ldpc_trials_syndromes_device(None, 1, p, None, None) == 1 and b"syndromes" in err()
    assert lib.ldpc_trials_syndromes_device(None, 1, p, p, None) == 1 and b"handle" in err()
    for entry, extra in ((lib.ldpc_trials_score_device, (None,)), (lib.ldpc_trials_score, ())):
        assert entry(None, -1, p, p, p, p, *extra) == 1 and b"batch" in err()
        assert entry(None, 1, None, p, p, p, *extra) == 1 and b"guesses" in err()
        assert entry(None, 1, p, None, p, p, *extra) == 1 and b"errors" in err()
        assert entry(None, 1, p, p, p, None, *extra) == 1 and b"counts" in err()
        assert entry(None, 1, p, p, None, p, *extra) == 1 and b"handle" in err()
    assert lib.ldpc_trials_destroy(None) == 0 and lib.ldpc_trials_kernel(None) == 0
    if lib.ldpc_device_count() == 0:
        assert create(2, 2, 2, cp, gp, 0, 0, None, None, None) == 2 and not h.value   # LDPC_ERR_NO_DEVICE, no CPU fallback
        with pytest.raises(ldpc.LdpcError) as ei:
            ldpc.Trials(ldpc.parity_check_matrix(96, 6, 3))
        assert ei.value.status == 2
