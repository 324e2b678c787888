"""The standard rule of the OSD step (ldpc_osd_set_search; include/ldpc_mi355x.h "THE STANDARD RULE"), what can be
checked without a GPU: the numpy model (tests/osd_search_model.py) against an independent brute force, the properties
of the search, the weight formula, the argument checks of the new entry, the host entry's refusal, the symbols and the
Python layer's errors."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
import relay_model
from osd_search_model import EXHAUSTIVE, SWEEP, candidates, eliminate, osd_search_model, search_order, weights_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- an independent brute force: integer bitmask rank, H e = syn solved by trying every e ------------------------------

def _rank(vectors):
    """Rank over GF(2) of integers read as bit vectors (an xor basis keyed by leading bit)."""
    basis = {}
    for v in vectors:
        while v:
            h = v.bit_length()
            if h not in basis:
                basis[h] = v
                break
            v ^= basis[h]
    return len(basis)


def _brute(Hd, syn, bp, llr, method, order, q):
    m, n = Hd.shape
    if all(int(Hd[i] @ bp) % 2 == int(syn[i] != 0) for i in range(m)):
        return np.array(bp, dtype=np.uint8), None, None
    # the order, by a plain comparison sort on (is NaN, value, index)
    perm = sorted(range(n), key=lambda j: (bool(np.isnan(llr[j])), 0.0 if np.isnan(llr[j]) or llr[j] == 0 else float(llr[j]), j))
    colint = [sum(int(Hd[i, j]) << i for i in range(m)) for j in range(n)]
    piv, chosen = [], []
    for c in perm:
        if _rank(chosen + [colint[c]]) > len(chosen):
            chosen.append(colint[c])
            piv.append(c)
    t = [c for c in perm if c not in piv]
    target = sum(int(syn[i] != 0) << i for i in range(m))
    best = None
    for idx, F in enumerate(candidates(method, order, len(t))):
        sols = []
        for bits in itertools.product((0, 1), repeat=len(piv)):     # every assignment of the pivot bits
            acc = 0
            for k in F:
                acc ^= colint[t[k]]
            for b, c in zip(bits, piv):
                if b:
                    acc ^= colint[c]
            if acc == target:
                sols.append(bits)
        assert len(sols) == 1, "the pivot bits of e(F) are unique"
        e = np.zeros(n, dtype=np.uint8)
        e[[t[k] for k in F]] = 1
        e[piv] = sols[0]
        cost = int((e.astype(np.int64) * q).sum())
        if best is None or (cost, idx) < best[:2]:
            best = (cost, idx, e)
    return best[2], sorted(piv), best[0]


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_brute_force_on_small_matrices(seed):
    rng = np.random.default_rng(seed)
    for trial in range(25):
        m, n = int(rng.integers(1, 7)), int(rng.integers(1, 13))
        Hd = (rng.random((m, n)) < 0.4).astype(np.uint8)
        if trial % 4 == 0 and m > 2:
            Hd[-1] = Hd[0] ^ Hd[1]                                  # a dependent row
        e0 = (rng.random(n) < 0.3).astype(np.uint8)
        syn = (Hd.astype(np.int64) @ e0) % 2
        bp = (rng.random(n) < 0.2).astype(np.uint8)
        llr = rng.choice([-2.5, -0.0, 0.0, 1.0, 3.5, np.inf, -np.inf, np.nan, 0.25], size=n) if trial % 2 else rng.normal(0, 3, n)
        q = np.ones(n, dtype=np.int64) if trial % 3 == 0 else weights_of(rng.choice([-1.0, 0.5, 2.0, 2.0, 7.25], size=n))
        for method, order in ((SWEEP, 0), (SWEEP, 2), (SWEEP, 5), (SWEEP, 64), (EXHAUSTIVE, 0), (EXHAUSTIVE, 1), (EXHAUSTIVE, 4)):
            want, piv, cost = _brute(Hd, syn, bp, llr, method, order, q)
            got, gcost = osd_search_model(Hd, syn, bp, llr, method, order, q, want_cost=True)
            assert np.array_equal(got, want), (seed, trial, method, order)
            if piv is not None:
                mp, mt, _, _ = eliminate(Hd, syn, search_order(llr))
                assert sorted(mp.tolist()) == piv and gcost == cost
                assert mp.size == _rank([sum(int(Hd[i, j]) << i for i in range(m)) for j in range(n)])
            assert np.array_equal((Hd.astype(np.int64) @ got) % 2, syn)


def _bb72():
    HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(HX)


_MS = {}


def _after_minsum():
    """BB-72 H_X, 400 syndromes of errors at 0.06 (seed 3), after the min-sum model at 30 iterations: the models' usual case."""
    if not _MS:
        from minsum_model import MinSumModel, llr_of_probs

        H = _bb72()
        E = ldpc.codes.random_errors(72, 400, 0.06, seed=3)
        syn = ldpc.codes.syndromes_of(H, E)
        err, conv, _, L = MinSumModel(H, llr_of_probs(np.full(72, 0.06)), 30).decode(syn)[:4]
        _MS["case"] = (H, np.asarray(H.todense()).astype(np.uint8), E, syn, err, conv, np.asarray(L, dtype=np.float64))
    return _MS["case"]


def test_sweep_never_costs_more_than_osd0_and_costs_fall_with_the_order():
    H, Hd, E, syn, err, conv, L = _after_minsum()
    q = weights_of(np.random.default_rng(1).choice([1.5, 2.75, 4.0], size=72))
    for weights in (None, q):
        for b in np.nonzero(conv == 0)[0][:40]:
            costs = []
            for lam in (0, 1, 2, 5, 10, 20, 64):
                e, c = osd_search_model(Hd, syn[b], err[b], L[b], SWEEP, lam, weights, want_cost=True)
                assert np.array_equal((Hd.astype(np.int64) @ e) % 2, syn[b])
                costs.append(c)
            assert all(x >= y for x, y in zip(costs, costs[1:])), costs
            ex = [osd_search_model(Hd, syn[b], err[b], L[b], EXHAUSTIVE, lam, weights, want_cost=True)[1] for lam in (0, 2, 6, 10)]
            # OSD-0 is candidate 0 alone (the exhaustive search at order 0); the sweep has its K single flips at every order
            assert costs[0] <= ex[0] and all(x >= y for x, y in zip(ex, ex[1:])), (ex, costs)


def test_logical_failures_on_bb72_after_minsum():
    """The counts DESIGN.md quotes: of 400 syndromes at 0.06, min-sum(30) alone, then reference OSD-0 (the model of the
    reference's rule), standard OSD-0 and CS-10 on what min-sum leaves.  A failure = the guess misses the syndrome or
    differs from the error by a logical operator (codes.css_logicals, as Trials.score counts block errors).  The counts
    are printed; asserted is what the construction guarantees: every OSD output reproduces its syndrome, so OSD leaves
    no failure of the first kind."""
    from osd_model import osd_model_postprocess

    H, Hd, E, syn, err, conv, L = _after_minsum()
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    Lz = np.asarray(sp.csc_matrix(ldpc.codes.css_logicals(HX, HZ)[1]).todense()).astype(np.int64)

    def failures(est):
        d = (E ^ est).astype(np.int64)
        return int((((d @ Hd.T.astype(np.int64)) % 2).any(axis=1) | ((d @ Lz.T) % 2).any(axis=1)).sum())

    ref0 = np.array([err[b] if conv[b] else osd_model_postprocess(Hd, syn[b], err[b], L[b], 0) for b in range(400)])
    std0 = np.array([osd_search_model(Hd, syn[b], err[b], L[b], EXHAUSTIVE, 0) for b in range(400)])
    cs10 = np.array([osd_search_model(Hd, syn[b], err[b], L[b], SWEEP, 10) for b in range(400)])
    for est in (ref0, std0, cs10):
        assert np.array_equal(ldpc.codes.syndromes_of(H, est), syn)
    print(f"unconverged {int((conv == 0).sum())}; failures of 400: min-sum(30) {failures(err)}, + reference OSD-0 {failures(ref0)}, "
          f"+ standard OSD-0 {failures(std0)}, + CS-10 {failures(cs10)}")


# ---- the C entry -------------------------------------------------------------------------------------------------------

def _handle(s, n, order=0):
    lib = ldpc._capi.lib()
    colptr = np.arange(n + 1, dtype=np.int64)
    rowval = (np.arange(n, dtype=np.int64) % s)
    h = ctypes.c_void_p()
    assert lib.ldpc_osd_create(s, n, n, colptr.ctypes.data, rowval.ctypes.data, order, ctypes.byref(h)) == 0
    return h


def test_weight_formula_equals_the_relays_on_its_edge_values():
    lib = ldpc._capi.lib()
    u = 2.0 ** -16
    llr = np.array([2.0 ** 24, 1e9, -2.0 ** 24, -1e9, 2.0 ** 24 - 0.5, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u,
                    0.0, -0.0, 1.0, -3.25, 0.49999 * u, 0.50001 * u, np.log(0.94 / 0.06)])
    want = [2 ** 40, 2 ** 40, -2 ** 40, -2 ** 40, 2 ** 40 - 32768, 0, 2, 2, 0, -2, -2, 0, 0, 65536, -212992, 0, 1]
    h = _handle(3, llr.size)
    assert lib.ldpc_osd_set_search(h, 2, 10, llr.size, llr.ctypes.data) == 0
    got = [int(lib.ldpc_osd_search_weight(h, j)) for j in range(llr.size)]
    assert got[:-1] == want
    assert got == weights_of(llr).tolist()
    # the relay decoder takes binary32 priors: on such values the two formulas are one
    l32 = llr.astype(np.float32).astype(np.float64)
    assert lib.ldpc_osd_set_search(h, 2, 10, llr.size, l32.ctypes.data) == 0
    assert [int(lib.ldpc_osd_search_weight(h, j)) for j in range(llr.size)] == relay_model.weights_of(l32).tolist()
    assert lib.ldpc_osd_destroy(h) == 0


def test_set_search_rejects_bad_arguments():
    lib = ldpc._capi.lib()
    n = 6
    ok = np.ones(n)
    h = _handle(2, n, order=3)
    assert lib.ldpc_osd_search_method(None) == 0 and lib.ldpc_osd_search_method(h) == 0
    assert lib.ldpc_osd_set_search(None, 2, 10, n, None) == 1 and b"NULL" in lib.ldpc_last_error()
    for method in (-1, 3):
        assert lib.ldpc_osd_set_search(h, method, 0, n, None) == 1 and b"method" in lib.ldpc_last_error()
    for method, order in ((1, -1), (1, 17), (2, -1), (2, 65), (0, 41)):
        assert lib.ldpc_osd_set_search(h, method, order, n, None) == 1 and b"order" in lib.ldpc_last_error()
    for bad_n in (n - 1, n + 1, 0):
        assert lib.ldpc_osd_set_search(h, 2, 10, bad_n, ok.ctypes.data) == 1 and b"columns" in lib.ldpc_last_error()
    for bad in (np.inf, -np.inf, np.nan):
        v = ok.copy()
        v[4] = bad
        assert lib.ldpc_osd_set_search(h, 2, 10, n, v.ctypes.data) == 1 and b"finite" in lib.ldpc_last_error()
    assert lib.ldpc_osd_set_search(h, 0, 3, n, ok.ctypes.data) == 1
    assert lib.ldpc_osd_search_method(h) == 0 and lib.ldpc_osd_search_weight(h, 0) == 1      # nothing changed
    for method, order in ((1, 16), (2, 64), (2, 0), (0, 40)):
        assert lib.ldpc_osd_set_search(h, method, order, n, None) == 0 and lib.ldpc_osd_search_method(h) == method
    assert lib.ldpc_osd_set_search(h, 2, 10, n, (-ok).ctypes.data) == 0 and lib.ldpc_osd_search_weight(h, 5) == -65536
    assert lib.ldpc_osd_destroy(h) == 0
    big = (1 << 22) + 1
    h = _handle(1, big)
    assert lib.ldpc_osd_set_search(h, 2, 10, big, None) == 5 and b"2^22" in lib.ldpc_last_error()
    assert lib.ldpc_osd_set_search(h, 1, 2, big, None) == 5
    assert lib.ldpc_osd_destroy(h) == 0


def test_host_entry_refuses_the_standard_rule_and_names_the_device_entry():
    H = _bb72()
    syn, e, L = np.zeros((2, 36), np.uint8), np.zeros((2, 72), np.uint8), np.zeros((2, 72))
    for method in ("exhaustive", "combination_sweep"):
        post = ldpc.OSDPostProcessor(H, 4, method=method)
        assert post.method == method and post._L.ldpc_osd_search_method(post._h) == ldpc.osd.OSD_METHODS[method]
        with pytest.raises(ldpc.LdpcError) as ei:
            post.postprocess(syn, e, L)
        assert ei.value.status == 5 and "ldpc_osd_postprocess_batch_device" in ei.value.message
        post.close()
    post = ldpc.OSDPostProcessor(H, 4)          # the default is the reference rule, host form included
    assert post.method == "reference" and post._L.ldpc_osd_search_method(post._h) == 0
    assert post.postprocess(syn, e, L).shape == (2, 72)
    post.close()


def test_a_prepared_handle_keeps_its_rule():
    """ldpc_osd_set_search comes before ldpc_osd_device_prepare.  (Needs a device to prepare: elsewhere the prepare call
    itself answers NO_DEVICE and the handle stays unprepared and settable.)"""
    lib = ldpc._capi.lib()
    post = ldpc.OSDPostProcessor(_bb72(), 2, method="combination_sweep")
    if lib.ldpc_device_count() == 0:
        with pytest.raises(ldpc.LdpcError) as ei:
            post.prepare_device()
        assert ei.value.status == 2 and post.kernel == 0
        assert lib.ldpc_osd_set_search(post._h, 1, 3, 72, None) == 0
    else:
        post.prepare_device(0)
        assert lib.ldpc_osd_set_search(post._h, 1, 3, 72, None) == 1 and b"already prepared" in lib.ldpc_last_error()
        assert lib.ldpc_osd_search_method(post._h) == 2
    post.close()


def _prototypes(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"^[ \t]*((?:const\s+)?\w+[\s\*]+)(ldpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        protos[m.group(2)] = (" ".join(m.group(1).split()), [a.strip() for a in m.group(3).split(",")])
    return protos


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_declared_exported_and_bound_as_declared(experiments):
    lib = ldpc._capi.lib(experiments)
    protos = _prototypes("ldpc_mi355x_osd_search.h")
    assert tuple(protos) == ("ldpc_osd_set_search", "ldpc_osd_search_method", "ldpc_osd_search_weight")
    assert tuple(protos) == ldpc._capi.OSD_SEARCH_SYMBOLS == tuple(ldpc._capi.OSD_SEARCH_API)
    hdr = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    assert '#include "ldpc_mi355x_osd_search.h"' in hdr
    assert "THE STANDARD RULE" in hdr[hdr.index("ldpc_osd_postprocess_batch_device("):hdr.index("ldpc_mi355x_osd_search.h")]
    jl = open(os.path.join(ROOT, "ldpcdecoders.jl_amd", "julia", "LDPCDecodersMI355X.jl")).read()
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "ldpc_status": ctypes.c_int32}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert ":%s" % name in jl
        assert fn.restype is scalars[ret], (name, ret)
        assert len(fn.argtypes) == len(args), (name, args)
        for got, arg in zip(fn.argtypes, args):
            if "*" in arg:
                assert got is ctypes.c_void_p, (name, arg, got)
            else:
                assert got is scalars[[w for w in arg.split() if w != "const"][0]], (name, arg, got)
    assert lib.ldpc_abi_version() == 4   # added by symbol


def test_python_layer_value_errors():
    H = _bb72()
    with pytest.raises(ValueError):
        ldpc.OSDPostProcessor(H, 2, method="cs")
    with pytest.raises(ValueError):
        ldpc.OSDPostProcessor(H, 2, weights=np.ones(72))                      # weights need the standard rule
    with pytest.raises(ValueError):
        ldpc.OSDPostProcessor(H, 2, method="combination_sweep", weights=np.ones(71))
    with pytest.raises(ldpc.LdpcError) as ei:
        ldpc.OSDPostProcessor(H, 65, method="combination_sweep")
    assert ei.value.status == 1
    with pytest.raises(ldpc.LdpcError):
        ldpc.OSDPostProcessor(H, 17, method="exhaustive")
    with pytest.raises(ldpc.LdpcError):
        ldpc.OSDPostProcessor(H, 2, method="exhaustive", weights=np.full(72, np.inf))
    ldpc.OSDPostProcessor(H, 64, method="combination_sweep", weights=-np.ones(72)).close()
    # the decoder: every check comes before a BP decoder (and so a device) is asked for
    for kw in (dict(osd_method="combination_sweep"), dict(osd_method="exhaustive", osd="host"),
               dict(osd_method="sweep", osd="device"), dict(osd_weights="priors"), dict(osd_weights=np.ones(72)),
               dict(osd_method="combination_sweep", osd="device", osd_weights="prior")):
        with pytest.raises(ValueError):
            ldpc.BeliefPropagationOSDDecoder(H, 0.05, 10, osd_order=2, **kw)


def test_set_search_under_sanitizers(tmp_path):
    """osd_host.cpp with AddressSanitizer + UBSan, driven by tests/native/osd_search_sanitize.cpp (a program of its own,
    CPU only): the argument checks, the weight table, the host entry's refusal."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "osd_search_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "osd_search_sanitize.cpp"),
                           os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc", "osd_host.cpp"), "-lpthread", "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
