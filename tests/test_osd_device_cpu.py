"""Device form of the OSD step, what can be checked without a GPU: the restated pm_exp, the CPU model of the stated
key rule (tests/osd_model.py) against the dense oracle on the true LLRs, the new symbols, and that the new entries
check their arguments before any device work."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from oracle import BPOracle, osd_oracle_postprocess
from osd_model import libm_order, model_order, osd_model_postprocess, pm_exp, surrogate_llr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bb72():
    HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(HX)


# (name, H, decoder per, error rate, iterations, syndromes, seed): the workloads the key rule was measured on
WORKLOADS = [
    ("bb72_005_004_s0", _bb72, 0.005, 0.04, 50, 4000, 0),
    ("bb72_005_004_s3", _bb72, 0.005, 0.04, 50, 4000, 3),
    ("bb72_003_003", _bb72, 0.03, 0.03, 50, 4000, 0),
    ("bb72_005_006_it20", _bb72, 0.005, 0.06, 20, 4000, 0),
    ("ldpc200_01", lambda: ldpc.codes.parity_check_csc(200, 10, 9), 0.1, 0.1, 50, 512, 0),
    ("ldpc1000_003", lambda: ldpc.codes.parity_check_csc(1000, 10, 9), 0.03, 0.03, 50, 256, 0),
    ("ldpc1000_02", lambda: ldpc.codes.parity_check_csc(1000, 10, 9), 0.2, 0.2, 50, 64, 0),
]
_CACHE = {}


def _workload(name):
    if name not in _CACHE:
        _, mk, per, rate, iters, B, seed = next(w for w in WORKLOADS if w[0] == name)
        H = sp.csc_matrix(mk())
        E = ldpc.codes.random_errors(H.shape[1], B, rate, seed=seed)
        syn = ldpc.codes.syndromes_of(H, E)
        oc = BPOracle(csc=(H.indptr, H.indices), shape=H.shape, per=per, max_iters=iters)
        err, conv, llr, _ = oc.batchdecode(syn)
        _CACHE[name] = (H, syn, err, llr)
    return _CACHE[name]


def _ulps(a, b):
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("name", [w[0] for w in WORKLOADS])
def test_pm_exp_restatement_within_2_ulp_of_libm(name):
    _, _, _, llr = _workload(name)
    v = np.unique(llr[np.isfinite(llr)])
    ref = np.array([math.exp(x) for x in v])
    d = _ulps(pm_exp(v), ref)
    print(f"{name}: {v.size} distinct LLRs, max {int(d.max())} ulp")
    assert d.max() <= 2
    assert np.isnan(pm_exp(np.array([np.nan]))[0]) and pm_exp(np.array([np.inf]))[0] == np.inf
    assert pm_exp(np.array([-np.inf]))[0] == 0.0 and pm_exp(np.array([0.0]))[0] == 1.0


def test_pm_exp_restatement_equals_the_c_function(tmp_path):
    """Bit for bit against csrc/portable_math.h itself (gcc, -ffp-contract=off)."""
    import shutil
    import subprocess

    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "pm.c"
    src.write_text('#include "portable_math.h"\nvoid pm_exp_many(long n, const double *x, double *y)'
                   '{ for (long i = 0; i < n; ++i) y[i] = pm_exp(x[i]); }\n')
    so = str(tmp_path / "pm.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), str(src), "-o", so])
    L = ctypes.CDLL(so)
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-40, 5, 200000), rng.uniform(-708, 709, 20000), -np.exp(rng.uniform(-30, 3, 50000)),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 709.5, -708.5]])
    y = np.empty_like(x)
    L.pm_exp_many(ctypes.c_long(x.size), ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data))
    assert np.array_equal(pm_exp(x).view(np.uint64), y.view(np.uint64))


def test_surrogate_realises_the_model_order_under_libm():
    rng = np.random.default_rng(2)
    for trial in range(50):
        n = int(rng.integers(1, 200))
        llr = -np.exp(rng.uniform(-12, 3, n))
        llr[rng.random(n) < 0.3] = rng.choice(llr)          # ties
        llr[rng.random(n) < 0.05] = 0.0
        llr[rng.random(n) < 0.05] = -np.inf
        llr[rng.random(n) < 0.05] = 3.0                     # p > 1: key p
        perm, cls = model_order(llr)
        sur = surrogate_llr(llr)
        assert np.array_equal(libm_order(sur), perm)
        # ... and the same ties: equal surrogates exactly inside a class
        assert np.array_equal(np.unique(sur[perm], return_inverse=True)[1].max() + 1, cls[-1] + 1)
        for a in range(n - 1):
            assert (sur[perm[a]] == sur[perm[a + 1]]) == (cls[a] == cls[a + 1])
    # a NaN orders last, by ascending index
    perm, _ = model_order(np.array([np.nan, -1.0, np.nan, -1e-9, np.inf]))
    assert perm.tolist() == [4, 3, 1, 0, 2]


@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("name", [w[0] for w in WORKLOADS])
def test_model_equals_the_oracle_where_the_orders_agree(name, order):
    """Equal in every element on every syndrome whose libm order equals the model's order; the others still satisfy
    H e = s and are at most 0.5 % of the workload (a condition: observed <= 0.05 %)."""
    H, syn, err, llr = _workload(name)
    Hd = np.asarray(H.todense()).astype(np.uint8)
    B = syn.shape[0]
    differ = 0
    for b in range(B):
        same_order = np.array_equal(libm_order(llr[b]), model_order(llr[b])[0])
        mod = osd_model_postprocess(Hd, syn[b], err[b], llr[b], order)
        if same_order:
            ref = osd_oracle_postprocess(Hd, syn[b], err[b], llr[b], order)
            assert np.array_equal(mod, ref), f"{name} order {order} syndrome {b}: the model differs from the oracle"
        else:
            differ += 1
            assert np.array_equal((Hd.astype(np.int64) @ mod.astype(np.int64)) % 2, syn[b])
    print(f"{name} order {order}: libm order differs from the model's on {differ} of {B} syndromes")
    assert differ <= 0.005 * B


def test_new_symbols_exported_and_declared():
    lib = ldpc._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    jl = open(os.path.join(ROOT, "ldpcdecoders.jl_amd", "julia", "LDPCDecodersMI355X.jl")).read()
    for sym in ("ldpc_osd_device_prepare", "ldpc_osd_device_kernel", "ldpc_osd_postprocess_batch_device"):
        assert sym in ldpc._capi.EXPORTED_SYMBOLS
        getattr(lib, sym)
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert ":%s" % sym in jl


def test_device_entries_validate_before_any_device_work():
    lib = ldpc._capi.lib()
    colptr = np.array([0, 2, 2], dtype=np.int64)
    rows = np.array([0, 1], dtype=np.int64)

    def make(order):
        h = ctypes.c_void_p()
        assert lib.ldpc_osd_create(2, 2, 2, colptr.ctypes.data, rows.ctypes.data, order, ctypes.byref(h)) == 0
        return h

    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.ldpc_osd_device_prepare(None, -1, 0) == 1 and b"NULL" in lib.ldpc_last_error()
    assert lib.ldpc_osd_device_kernel(None) == 0
    assert lib.ldpc_osd_postprocess_batch_device(None, 1, p, p, p, p, None) == 1
    h = make(0)
    assert lib.ldpc_osd_device_kernel(h) == 0
    for variant in (-1, 4, 9):
        assert lib.ldpc_osd_device_prepare(h, -1, variant) == 1 and b"kernel_variant" in lib.ldpc_last_error()
    assert lib.ldpc_osd_postprocess_batch_device(h, -1, p, p, p, p, None) == 1 and b"negative" in lib.ldpc_last_error()
    assert lib.ldpc_osd_postprocess_batch_device(h, 1, p, p, p, p, None) == 1 and b"not prepared" in lib.ldpc_last_error()
    assert lib.ldpc_osd_postprocess_batch_device(h, 0, p, p, p, p, None) == 1   # unprepared, even for an empty batch
    assert lib.ldpc_osd_destroy(h) == 0
    # an order whose candidate loop the device entry does not run (bound 16; the host entry takes up to 40)
    h = make(17)
    assert lib.ldpc_osd_device_prepare(h, -1, 0) == 5 and b"osd_order" in lib.ldpc_last_error()
    assert lib.ldpc_osd_device_kernel(h) == 0
    assert lib.ldpc_osd_destroy(h) == 0
    # a forced on-chip tier that the graph does not fit
    big = ldpc.OSDPostProcessor(ldpc.codes.parity_check_csc(4000, 10, 5), 0)
    for variant in (1, 2):
        assert lib.ldpc_osd_device_prepare(big._h, -1, variant) == 5 and b"does not fit" in lib.ldpc_last_error()
    mid = ldpc.OSDPostProcessor(ldpc.codes.parity_check_csc(1000, 10, 9), 0)
    assert lib.ldpc_osd_device_prepare(mid._h, -1, 1) == 5
    if lib.ldpc_device_count() == 0:
        # no device: the opt-in form fails loudly, it never computes on the CPU
        assert lib.ldpc_osd_device_prepare(mid._h, -1, 0) == 2
        with pytest.raises(ldpc.LdpcError) as ei:
            mid.prepare_device()
        assert ei.value.status == 2 and mid.kernel == 0
    with pytest.raises(ValueError):
        ldpc.BeliefPropagationOSDDecoder(ldpc.codes.parity_check_csc(96, 6, 3), 0.01, 5, osd="gpu")
