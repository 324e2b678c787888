"""The Python host layer without a GPU: every prototype of the two headers against the binding table, the handle base
(against a stub library and against the real one), the prior parser and the device-tensor check."""
import ctypes
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ldpcdecoders_jl_amd as ldpc
from ldpcdecoders_jl_amd import _capi, _host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("ldpc_mi355x.h", "ldpc_mi355x_debug.h")


# ---- 1. the headers against the binding -----------------------------------------------------------------------------------

def _prototypes(header):
    """name -> (return type, [argument, ...]) of every function the header declares."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    protos = {}
    for m in re.finditer(r"^[ \t]*((?:const\s+)?\w+[\s\*]+)(ldpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        args = [a.strip() for a in m.group(3).split(",")]
        protos[m.group(2)] = (" ".join(m.group(1).split()), [] if args == ["void"] else args)
    return protos


SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double,
           "ldpc_status": ctypes.c_int32}


def _kind(decl):
    """"pointer", or the ctypes scalar, of an argument or return declaration."""
    if "*" in decl or "[" in decl:
        return "pointer"
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def test_the_parser_finds_every_function_of_both_headers():
    main, debug = (_prototypes(h) for h in HEADERS)
    assert len(main) == 95 and len(debug) == 13 and not set(main) & set(debug)
    assert main["ldpc_abi_version"] == ("int32_t", []) and main["ldpc_last_error"] == ("const char *", [])
    assert main["ldpc_bp_call_phase_ticks"][1][-1] == "uint64_t ticks[3]" and debug["ldpc_debug_process_state"] == ("void *", [])


def test_the_symbol_tuples_are_the_tables_keys():
    main, debug = (_prototypes(h) for h in HEADERS)
    assert isinstance(_capi.EXPORTED_SYMBOLS, tuple) and isinstance(_capi.DEBUG_SYMBOLS, tuple)
    assert _capi.EXPORTED_SYMBOLS == tuple(_capi.API) and _capi.DEBUG_SYMBOLS == tuple(_capi.DEBUG_API)
    assert set(_capi.EXPORTED_SYMBOLS) | set(_capi.DEBUG_SYMBOLS) == set(_capi.API) | set(_capi.DEBUG_API)
    assert set(_capi.API) == set(main) and set(_capi.DEBUG_API) == set(debug)
    assert len(set(_capi.EXPORTED_SYMBOLS + _capi.DEBUG_SYMBOLS)) == 108


@pytest.mark.parametrize("experiments", [False, True])
def test_every_function_is_bound_as_its_header_declares_it(experiments):
    L = _capi.lib(experiments)
    protos = {**_prototypes(HEADERS[0]), **_prototypes(HEADERS[1])}
    assert len(protos) == 108
    for name, (ret, args) in protos.items():
        fn = getattr(L, name)                                    # (exported by this build)
        want = _kind(ret)
        if want == "pointer":
            assert fn.restype is (ctypes.c_char_p if "char" in ret else ctypes.c_void_p), (name, ret, fn.restype)
        else:
            assert fn.restype is want, (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), (name, args, fn.argtypes)
        for got, arg in zip(fn.argtypes, args):
            want = _kind(arg)
            if want == "pointer":
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, arg, got)
            else:
                assert got is want, (name, arg, got)


# ---- 2. the handle base against a stub library ------------------------------------------------------------------------------

class StubLib:
    """Counts what a handle class calls."""

    def __init__(self, status=0, handle=0x1234):
        self.status, self.handle, self.created, self.destroyed = status, handle, 0, []

    def stub_create(self, a, b, out):
        assert (a, b) == (7, 8)
        self.created += 1
        if self.status == 0:
            out._obj.value = self.handle
        return self.status

    def stub_destroy(self, h):
        self.destroyed.append(h.value)
        return 0

    def ldpc_last_error(self):
        return b"stub says no"


class Owner(_host.Handle):
    _destroy = "stub_destroy"

    def __init__(self, L, fail_before_binding=False):
        if fail_before_binding:
            raise ValueError("refused")
        self._create(L, L.stub_create, 7, 8)


@pytest.fixture
def unraisable(monkeypatch):
    seen = []
    monkeypatch.setattr(sys, "unraisablehook", lambda u: seen.append(u))
    return seen


def test_destroy_is_called_exactly_once(unraisable):
    L = StubLib()
    o = Owner(L)
    assert o._L is L and o._h.value == 0x1234 and L.created == 1 and L.destroyed == []
    o.close()
    assert o._h is None and L.destroyed == [0x1234]
    o.close()
    del o
    gc.collect()
    assert L.destroyed == [0x1234] and unraisable == []
    o = Owner(L)                                                 # ... and by __del__ alone where nobody closed
    del o
    gc.collect()
    assert L.destroyed == [0x1234, 0x1234] and unraisable == []


def test_destroy_is_never_called_with_a_null_handle(unraisable):
    L = StubLib(status=1)                                        # a create that fails leaves nothing to free
    with pytest.raises(ldpc.LdpcError) as ei:
        Owner(L)
    assert ei.value.status == 1 and "stub says no" in str(ei.value)
    L = StubLib(handle=0)                                        # neither does one that answered OK with a NULL handle
    o = Owner(L)
    assert not o._h
    o.close()
    del o, ei
    gc.collect()
    assert L.destroyed == [] and unraisable == []


def test_del_is_silent_after_a_constructor_that_raised_before_binding(unraisable):
    with pytest.raises(ValueError):
        Owner(StubLib(), fail_before_binding=True)
    o = Owner.__new__(Owner)
    assert o._h is None and o._L is None
    o.close()
    o.__del__()
    del o
    gc.collect()
    assert unraisable == []


def test_every_handle_class_is_on_the_base_and_names_its_destroy():
    classes = (ldpc.BeliefPropagationDecoder, ldpc.BPOTSDecoder, ldpc.BitFlipDecoder, ldpc.MinSumDecoder, ldpc.RelayMinSumDecoder,
               ldpc.PauliMinSumDecoder, ldpc.Trials, ldpc.CSSTrials, ldpc.OSDPostProcessor, ldpc.WindowStep)
    for c in classes:
        assert issubclass(c, _host.Handle) and c._destroy in _capi.API and c._destroy.endswith("_destroy"), c
        assert c.__del__ is _host.Handle.__del__
        assert (c.close is _host.Handle.close) == (c is not ldpc.BeliefPropagationDecoder)   # BP: the multi-device variant
    assert len({c._destroy for c in classes}) == 10


# ---- 3. the same against the real library -----------------------------------------------------------------------------------

CONSTRUCTIONS = {
    "BeliefPropagationDecoder": "ldpc.BeliefPropagationDecoder(H, 0.05, 5)",
    "BPOTSDecoder": "ldpc.BPOTSDecoder(H, 0.05, 5)",
    "BitFlipDecoder": "ldpc.BitFlipDecoder(H, 0.05, 5)",
    "MinSumDecoder": "ldpc.MinSumDecoder(H, 0.05, 5)",
    "RelayMinSumDecoder": "ldpc.RelayMinSumDecoder(H, 0.05, 5, legs=2)",
    "PauliMinSumDecoder": "ldpc.PauliMinSumDecoder(H, H, 0.05, 5)",
    "Trials": "ldpc.Trials(H)",
    "CSSTrials": "ldpc.CSSTrials(H, H)",
    "OSDPostProcessor": "ldpc.OSDPostProcessor(H, 0)",
    "WindowStep": "ldpc.WindowStep(H, [[0, 1, 2]], [list(range(7))], [list(range(7))])",
}
CHILD = """
import numpy as np
import ldpcdecoders_jl_amd as ldpc
H = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)   # Hamming (7, 4); Steane
try:
    obj = {expr}
except ldpc.LdpcError as e:
    print("status", e.status)
else:
    obj.close()
    obj.close()
    print("built and closed")
"""


def test_a_failed_or_finished_construction_leaves_nothing_for_the_interpreter_to_report():
    """Each of the ten classes in a process of its own: LDPC_ERR_NO_DEVICE without a GPU (OSDPostProcessor needs none), a
    handle that closes twice with one; and not a word on stderr either way ("Exception ignored in ... __del__")."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    names = list(CONSTRUCTIONS)
    results = {}
    for wave in (names[:5], names[5:]):                          # (five at a time: the children may each open a GPU)
        procs = {n: subprocess.Popen([sys.executable, "-c", CHILD.format(expr=CONSTRUCTIONS[n])], env=env, text=True,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE) for n in wave}
        for n, p in procs.items():
            out, err = p.communicate(timeout=300)
            results[n] = (p.returncode, out.strip(), err)
    no_gpu = _capi.lib().ldpc_device_count() == 0
    for n, (code, out, err) in results.items():
        want = "status 2" if no_gpu and n != "OSDPostProcessor" else "built and closed"
        assert (code, out, err) == (0, want, ""), (n, code, out, err)


# ---- 4. the prior parser ------------------------------------------------------------------------------------------------------

def test_the_three_spellings_of_a_uniform_prior_give_the_same_array():
    n = 11
    for p in (0.05, 0.3, 1e-4, np.float64(0.01)):
        a = _host.channel_prior(n, per=p)
        b = _host.channel_prior(n, channel_probs=[p] * n)
        c = _host.channel_prior(n, channel_llr=np.full(n, np.log((1 - p) / p)))
        for x in (a, b, c):
            assert x.dtype == np.float32 and x.shape == (n,) and x.flags.c_contiguous
        assert a.tobytes() == b.tobytes() == c.tobytes()
        assert a.tobytes() == ldpc.minsum.llr_of_probs(np.full(n, p)).tobytes()
    assert _host.channel_prior(0, per=0.1).shape == (0,)


def test_the_prior_parser_refuses_what_the_constructors_refused():
    one = "give exactly one of per, channel_probs and channel_llr"
    for kw in ({}, {"per": 0.1, "channel_probs": [0.1] * 4}, {"per": 0.1, "channel_llr": [1.0] * 4},
               {"channel_probs": [0.1] * 4, "channel_llr": [1.0] * 4}, {"per": 0.1, "channel_probs": [0.1] * 4, "channel_llr": [1.0] * 4}):
        with pytest.raises(TypeError, match=one):
            _host.channel_prior(4, **kw)
        with pytest.raises(TypeError, match=one):
            _host.one_prior_given(kw.get("per"), kw.get("channel_probs"), kw.get("channel_llr"))
    for per in (1, True, "0.1"):
        with pytest.raises(TypeError, match="per must be a Float64"):
            _host.channel_prior(4, per=per)
    for kw in ({"channel_probs": [0.1] * 3}, {"channel_llr": [1.0] * 5}, {"channel_llr": [[1.0] * 4]}, {"channel_probs": 0.1}):
        with pytest.raises(ValueError, match="one prior per bit: expected 4 entries"):
            _host.channel_prior(4, **kw)
    for kw in ({"per": 0.0}, {"per": 1.0}, {"per": -0.1}, {"per": float("nan")}, {"channel_probs": [0.1, 0.2, 1.5, 0.1]},
               {"channel_probs": [0.1, 0.0, 0.1, 0.1]}, {"channel_probs": [0.1, np.nan, 0.1, 0.1]}):
        with pytest.raises(ValueError, match="strictly inside"):
            _host.channel_prior(4, **kw)


def test_the_option_checks_keep_their_texts():
    assert _host.as_int(np.int64(3), "legs") == 3 and type(_host.as_int(np.int32(3), "legs")) is int
    for bad in (True, 3.0, "3", None):
        with pytest.raises(TypeError, match="^legs must be an Int$"):
            _host.as_int(bad, "legs")
    with pytest.raises(TypeError, match=r"^max_iters must be an Int \(reference signature: max_iters::Int\)$"):
        _host.as_int(2.0, "max_iters", " (reference signature: max_iters::Int)")
    _host.refuse_zero_alpha_clip(0.75, 1e6)
    for alpha, clip in ((0.0, 1e6), (0.75, 0.0), (1e-60, 1.0)):                          # (1e-60 is a zero as a float32)
        with pytest.raises(ldpc.LdpcError, match="got a zero") as ei:
            _host.refuse_zero_alpha_clip(alpha, clip)
        assert ei.value.status == 1
    assert _host.device_option(None) == -1 and _host.device_option(np.int64(3)) == 3
    assert ldpc.minsum._current_device is _host.current_device and ldpc.trials._current_device is _host.current_device


def test_the_host_preparation():
    with pytest.raises(AssertionError, match="^syndrome length does not match the number of checks$"):
        _host.host_batch(np.zeros((2, 4), dtype=np.uint8), 3, 7)
    with pytest.raises(AssertionError, match="^syndrome length does not match the number of checks$"):
        _host.host_syndromes(np.zeros(3, dtype=np.uint8), 3)
    syn, B, err, conv, llr, its = _host.host_batch(np.asfortranarray(np.ones((5, 3), dtype=np.int64)), 3, 7)
    assert B == 5 and syn.dtype == np.uint8 and syn.flags.c_contiguous and syn.all() and llr is None
    assert [(x.shape, x.dtype) for x in (err, conv, its)] == [((5, 7), np.uint8), ((5,), np.uint8), ((5,), np.int32)]
    llr = _host.host_batch(syn, 3, 7, want_llr=True)[4]
    assert llr.shape == (5, 7) and llr.dtype == np.float64 and llr.flags.c_contiguous
    assert _host.host_ptr(None) is None and _host.host_ptr(llr) == llr.ctypes.data
    colptr, rowval = _host.csc_arrays(ldpc.decoder._pattern_of(np.eye(3)))
    assert colptr.dtype == rowval.dtype == np.int64 and colptr.tolist() == [0, 1, 2, 3] and rowval.tolist() == [0, 1, 2]
    pat = _host.css_pattern(ldpc.decoder._pattern_of(np.ones((2, 3))))
    assert (pat.rows, pat.nnz) == (2, 6) and pat.colptr == pat.arrays[0].ctypes.data and pat.rowval == pat.arrays[1].ctypes.data
    assert ldpc.decoder._pattern_of is _host._pattern_of and ldpc.decoder.syndrome_bytes is _host.syndrome_bytes is ldpc.syndrome_bytes


# ---- 5. the tensor check, on CPU tensors ------------------------------------------------------------------------------------

def test_the_tensor_check_refuses_with_an_assertion_error():
    torch = pytest.importorskip("torch")
    good = torch.zeros((3, 4), dtype=torch.uint8)
    bad = {"a CPU tensor": (good, torch.uint8, (3, 4)),
           "a wrong dtype": (torch.zeros((3, 4), dtype=torch.int32), torch.uint8, (3, 4)),
           "a transposed view": (torch.zeros((4, 3), dtype=torch.uint8).t(), torch.uint8, (3, 4)),
           "a wrong shape": (good, torch.uint8, (4, 3)),
           "a wrong element count": (good, torch.uint8, 11)}
    assert not bad["a transposed view"][0].is_contiguous() and tuple(bad["a transposed view"][0].shape) == (3, 4)
    for what, (x, dtype, shape) in bad.items():
        for optional in (False, True):
            with pytest.raises(AssertionError):
                _host.tensor_ptr(x, dtype, shape, optional=optional)
    assert _host.tensor_ptr(None, torch.uint8, (3, 4), optional=True) is None
    with pytest.raises(AttributeError):
        _host.tensor_ptr(None, torch.uint8, (3, 4))                                      # a required tensor is not optional
    assert _host.stream_ptr(77, None).value == 77                                        # a given stream is taken as it is
