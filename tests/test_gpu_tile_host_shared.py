"""The host paths that the five decoders of the min-sum family share (csrc/tile_host.hpp, csrc/relay_host.hpp), pinned from
outside the library: one table of decoders, entries and arguments, and every case runs over all of it through the C entry
points -- the argument check of an entry (statuses and the exact texts), a handle on which no iteration runs, a grid
capped to one workgroup, two handles of different decoders taking turns on two streams, and the create-time texts of the
legs of the two relay decoders in the order the creates check them.  The graphs are the smallest that have every array:
s = 3, n = 6, and rx = rz = 2, n = 6 for the Pauli pair; the state of a syndrome is a few hundred bytes, so a tile is 64
syndromes wide.  Results are compared with the numpy models of tests/ (no tolerance: the rules have no division).

What other files assert already, on larger graphs, is not repeated here: the eight masks of optional outputs and slices
of a batch (test_gpu_relay.py, test_gpu_decim.py, test_gpu_pauli.py, test_gpu_pauli_relay.py, test_gpu_minsum.py) and
several tiles in one slot at other caps and widths (test_gpu_minsum_tiles.py, test_gpu_decim_widths.py,
test_gpu_pauli_relay.py, test_gpu_priors.py, test_gpu_layered.py).  The Pauli min-sum decoder reads no environment
variable, so the capped grid has no case for it."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as sp

import priors_model as pm
from decim_model import DecimModel
from minsum_model import MinSumModel
from pauli_model import PauliMinSumModel
from pauli_relay_model import PauliRelayModel
from relay_model import RelayModel

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID = 0, 1

H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1]], dtype=np.uint8)
HX = np.array([[1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 1, 1]], dtype=np.uint8)
HZ = np.array([[1, 1, 0, 0, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=np.uint8)      # every row meets every Hx row in 2 or 4 qubits
S, RX, RZ, N = 3, 2, 2, 6
LLR = np.array([2.0, 1.5, 2.5, 1.0, 3.0, 0.75], dtype=F)
IF0, IF1 = LLR + F(0.5), LLR - F(1.25)
PRIORS = np.array([[3.0, 2.5, 3.5, 2.0, 4.0, 1.75], [3.25, 2.75, 3.75, 2.25, 4.25, 2.0], [2.75, 2.25, 3.25, 1.5, 3.5, 1.25]], dtype=F)
GAMMAS = np.array([[0.125] * 6, [-0.2, 0.5, 0.0, 0.3, 0.1, 0.6]], dtype=F)
LEGS, STOP_AFTER, ITERS, ROUND, MAX_DEC = [3, 2], 2, 5, 3, 2

# An argument of an entry, in the order of the C signature: io "in" | "out"; `width` elements of `dtype` per syndrome;
# `null` the text when it alone is NULL at batch > 0, None where it may be NULL.
A = namedtuple("A", "name io dtype width null")
NBP = "NULL batch pointer"
Spec = namedtuple("Spec", "name prefix create entries model knob")


def _csc(M):
    C = sp.csc_matrix(M)
    C.sort_indices()
    return np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int64)


def _made(L, st, h):
    assert st == OK and h.value, (st, L.ldpc_last_error().decode())
    return h


def _binary(prefix, options, extra):
    """create(L, idle) of a decoder over H: extra(idle) -> the arguments between channel_llr and the options."""
    def create(L, idle):
        colptr, rowval = _csc(H)
        o = options()
        o.device = 0
        h = ctypes.c_void_p()
        keep = extra(idle)
        args = [k.ctypes.data if isinstance(k, np.ndarray) else k for k in keep]
        return _made(L, getattr(L, prefix + "_create")(S, N, len(rowval), colptr.ctypes.data, rowval.ctypes.data, LLR.ctypes.data, *args,
                                                       ctypes.byref(o), ctypes.byref(h)), h)
    return create


def _css(prefix, options, extra, ldpc):
    def create(L, idle):
        from ldpcdecoders_jl_amd._host import _pattern_of, css_pattern

        px, pz = css_pattern(_pattern_of(HX)), css_pattern(_pattern_of(HZ))
        o = options()
        o.device = 0
        if hasattr(o, "stop_after"):
            o.stop_after = STOP_AFTER
        h = ctypes.c_void_p()
        keep = extra(idle)
        args = [k.ctypes.data if isinstance(k, np.ndarray) else k for k in keep]
        return _made(L, getattr(L, prefix + "_create")(N, ctypes.byref(px), ctypes.byref(pz), PRIORS[0].ctypes.data, PRIORS[1].ctypes.data,
                                                       PRIORS[2].ctypes.data, *args, ctypes.byref(o), ctypes.byref(h)), h)
    return create


def _legs(idle):
    return [2, GAMMAS, np.array([0, 0] if idle else LEGS, dtype=np.int32)]


def _relay_options(ldpc):
    def options():
        o = ldpc._capi.RelayOptions()
        o.stop_after = STOP_AFTER
        return o
    return options


def _minsum_create(ldpc):
    plain = _binary("ldpc_minsum", ldpc._capi.MinSumOptions, lambda idle: [0 if idle else ITERS])

    def create(L, idle):
        h = plain(L, idle)
        assert L.ldpc_minsum_set_conditional_priors(h, IF0.ctypes.data, IF1.ctypes.data) == OK
        return h
    return create


def _named(names, values):
    """A model's tuple under the names of the entry's outputs; the LLRs as the float64 the library writes."""
    out = dict(zip(names, values))
    out["llr"] = np.ascontiguousarray(out["llr"], dtype=np.float64)
    return out


@functools.lru_cache(maxsize=None)
def table():
    import ldpcdecoders_jl_amd as ldpc

    syn, err, conv = A("syn", "in", np.uint8, S, NBP), A("err", "out", np.uint8, N, NBP), A("conv", "out", np.uint8, 1, NBP)
    llr, its = A("llr", "out", np.float64, N, None), A("iters", "out", np.int32, 1, None)
    sides = [A("sx", "in", np.uint8, RX, NBP), A("sz", "in", np.uint8, RZ, NBP), A("gx", "out", np.uint8, N, NBP),
             A("gz", "out", np.uint8, N, NBP), conv, A("llr", "out", np.float64, 3 * N, None), its]
    sol, dec = A("solutions", "out", np.int32, 1, None), A("decimated", "out", np.int32, 1, None)
    binary = ("err", "conv", "iters", "llr")
    return [
        Spec("minsum", "ldpc_minsum", _minsum_create(ldpc),
             {"decode_batch": [syn, err, conv, llr, its],
              "decode_batch_priors": [syn, A("priors", "in", F, N, "priors pointer is NULL"), err, conv, llr, its],
              "decode_batch_given": [syn, A("given", "in", np.uint8, N, "given pointer is NULL"), err, conv, llr, its]},
             {"decode_batch": lambda x: _named(binary, MinSumModel(H, LLR, ITERS).decode(x["syn"])),
              "decode_batch_priors": lambda x: _named(binary, pm.model_of("flooding", H, ITERS).decode(x["syn"], x["priors"])),
              "decode_batch_given": lambda x: _named(binary, pm.model_of("flooding", H, ITERS).decode(x["syn"], pm.select_priors(x["given"], IF0, IF1)))},
             True),
        Spec("relay", "ldpc_relay", _binary("ldpc_relay", _relay_options(ldpc), _legs), {"decode_batch": [syn, err, conv, llr, its, sol]},
             {"decode_batch": lambda x: _named(("err", "conv", "iters", "solutions", "llr"),
                                               RelayModel(H, LLR, GAMMAS, LEGS, stop_after=STOP_AFTER).decode(x["syn"]))}, True),
        Spec("decim", "ldpc_decim", _binary("ldpc_decim", ldpc._capi.DecimOptions, lambda idle: [0 if idle else ROUND, MAX_DEC]),
             {"decode_batch": [syn, err, conv, llr, its, dec]},
             {"decode_batch": lambda x: _named(("err", "conv", "iters", "decimated", "llr"), DecimModel(H, LLR, ROUND, MAX_DEC).decode(x["syn"]))}, True),
        Spec("pauli", "ldpc_pauli_minsum", _css("ldpc_pauli_minsum", ldpc._capi.PauliMinSumOptions, lambda idle: [0 if idle else ITERS], ldpc),
             {"decode_batch": sides},
             {"decode_batch": lambda x: _named(("gx", "gz", "conv", "iters", "llr"), PauliMinSumModel(HX, HZ, PRIORS, ITERS).decode(x["sx"], x["sz"]))},
             False),
        Spec("pauli_relay", "ldpc_pauli_relay", _css("ldpc_pauli_relay", ldpc._capi.PauliRelayOptions, _legs, ldpc), {"decode_batch": sides + [sol]},
             {"decode_batch": lambda x: _named(("gx", "gz", "conv", "iters", "solutions", "llr"),
                                               PauliRelayModel(HX, HZ, PRIORS, GAMMAS, LEGS, stop_after=STOP_AFTER).decode(x["sx"], x["sz"]))}, True),
    ]


NAMES = ["minsum", "relay", "decim", "pauli", "pauli_relay"]


def spec_of(name):
    return table()[NAMES.index(name)]


def inputs_of(rows, seed=5):
    """Every input any entry takes, `rows` syndromes of it: syndromes of sparse errors, priors around LLR, given bits."""
    rng = np.random.default_rng(seed)
    e, ez = (rng.random((rows, N)) < 0.2).astype(np.uint8), (rng.random((rows, N)) < 0.2).astype(np.uint8)
    return {"syn": (e @ H.T % 2).astype(np.uint8), "sx": (ez @ HX.T % 2).astype(np.uint8), "sz": (e @ HZ.T % 2).astype(np.uint8),
            "priors": (LLR[None, :] + rng.uniform(-0.5, 0.5, (rows, N))).astype(F), "given": (rng.random((rows, N)) < 0.3).astype(np.uint8)}


def call(L, spec, entry, h, batch, rows, device, null=(), stream=None, inputs=None):
    """One call of an entry on buffers of `rows` syndromes, the outputs pre-filled with 0xAB bytes -> (status, text,
    {output: array}); with `stream`, the outputs are read only once the device has drained."""
    import torch

    inputs = inputs if inputs is not None else inputs_of(rows)
    host = {}
    for a in spec.entries[entry]:
        if a.io == "in":
            host[a.name] = np.array(inputs[a.name][:rows], dtype=a.dtype, order="C")
        else:
            host[a.name] = np.full(rows * a.width * np.dtype(a.dtype).itemsize, 0xAB, dtype=np.uint8).view(a.dtype)
    held = {k: torch.from_numpy(v).cuda() for k, v in host.items()} if device else host
    torch.cuda.synchronize()
    ptr = (lambda k: held[k].data_ptr()) if device else (lambda k: host[k].ctypes.data)
    argv = [None if a.name in null else ptr(a.name) for a in spec.entries[entry]]
    fn = getattr(L, f"{spec.prefix}_{entry}" + ("_device" if device else ""))
    st = fn(h, batch, *argv, *([stream] if device else []))
    text = L.ldpc_last_error().decode() if st != OK else ""
    return st, text, (lambda: {a.name: (held[a.name].cpu().numpy() if device else host[a.name]) for a in spec.entries[entry] if a.io == "out"})


def outputs(result):
    import torch

    st, text, read = result
    assert st == OK, text
    torch.cuda.synchronize()
    return read()


def untouched(out):
    return all((v.view(np.uint8) == 0xAB).all() for v in out.values())


def same(got, want, what):
    for k, w in want.items():
        g = got[k].reshape(w.shape)
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), f"{what}: {k} differs"


def last_grid(L, spec, h):
    return getattr(L, spec.prefix + "_last_grid")(h)


def destroy(L, spec, h):
    assert getattr(L, spec.prefix + "_destroy")(h) == OK


# ---- the check of an entry's arguments ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_null_decoder_negative_batch_batch_zero_and_each_required_pointer(ldpc, gpu, name):
    """In the order the entries check: the decoder, the sign of the batch, batch = 0 (LDPC_OK with every pointer NULL,
    nothing written), then each required pointer NULL in turn at batch = 1.  Nothing is launched, no output is written."""
    import torch

    L, spec = gpu, spec_of(name)
    h = spec.create(L, False)
    for entry, args in spec.entries.items():
        for device in (True, False):
            what = f"{name} {entry} {'device' if device else 'host'} entry"
            st, text, out = call(L, spec, entry, None, 1, 4, device)
            assert (st, text) == (INVALID, "decoder is NULL") and untouched(out()), what
            st, text, out = call(L, spec, entry, h, -1, 4, device)
            assert (st, text) == (INVALID, "negative batch") and untouched(out()), what
            assert call(L, spec, entry, h, 0, 4, device, null=[a.name for a in args])[0] == OK, what
            st, text, out = call(L, spec, entry, h, 0, 4, device)
            torch.cuda.synchronize()
            assert st == OK and untouched(out()), what
            for a in args:
                st, text, out = call(L, spec, entry, h, 1, 4, device, null=[a.name])
                if a.null is None:
                    assert st == OK, (what, a.name, text)
                    continue
                torch.cuda.synchronize()
                assert (st, text) == (INVALID, a.null) and untouched(out()), (what, a.name, st, text)
    before = last_grid(L, spec, h)
    assert call(L, spec, "decode_batch", h, 1, 4, True, null=["conv"])[0] == INVALID and last_grid(L, spec, h) == before
    destroy(L, spec, h)


# ---- no iteration runs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_a_handle_on_which_no_iteration_runs_zeroes_every_output(ldpc, gpu, name):
    """max_iters = 0, round_iters = 0, every leg of 0 iterations: 65 syndromes (a tile and a lane) through every entry,
    every output -- the optional ones included -- zero where 0xAB was; no kernel ran."""
    L, spec = gpu, spec_of(name)
    h = spec.create(L, True)
    for entry in spec.entries:
        for device in (True, False):
            out = outputs(call(L, spec, entry, h, 65, 65, device))
            assert len(out) >= 4 and all(not v.view(np.uint8).any() for v in out.values()), (name, entry, device)
    assert last_grid(L, spec, h) == 0
    destroy(L, spec, h)


# ---- one workgroup for three tiles ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def model_of(name, entry, rows):
    want = spec_of(name).model[entry](inputs_of(rows))
    for v in want.values():
        v.setflags(write=False)
    return want


@pytest.mark.parametrize("name", [n for n in NAMES if n != "pauli"])
def test_a_grid_capped_to_one_workgroup_gives_the_results_of_an_uncapped_one(ldpc, gpu, monkeypatch, name):
    """LDPC_MS_GRID_MAX = 1 (read at create, experiments build): 130 syndromes are three tiles on one workgroup, and every
    entry gives what an uncapped handle gives and what the model gives, element for element."""
    spec = spec_of(name)
    X = ldpc._capi.lib(True)
    free = spec.create(X, False)
    monkeypatch.setenv("LDPC_MS_GRID_MAX", "1")
    capped = spec.create(X, False)
    monkeypatch.delenv("LDPC_MS_GRID_MAX")
    for entry in spec.entries:
        want = model_of(name, entry, 130)
        assert 0 < want["conv"].sum() and len(set(want["iters"].tolist())) > 1, (name, entry)
        for device in (True, False):
            got = outputs(call(X, spec, entry, capped, 130, 130, device))
            assert last_grid(X, spec, capped) == 1
            same(got, outputs(call(X, spec, entry, free, 130, 130, device)), f"{name} {entry}, capped against uncapped")
            assert last_grid(X, spec, free) == 3
            same(got, want, f"{name} {entry}, capped against the model")
    destroy(X, spec, capped)
    destroy(X, spec, free)


# ---- two handles, two streams -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", NAMES)
def test_two_decoders_taking_turns_on_two_streams_give_what_each_gives_alone(ldpc, gpu, first):
    """Each handle sees its calls arrive on alternating streams (the call order of a handle holds across streams: its
    workspace and LDS state are shared), while the other decoder runs on the other stream."""
    import torch

    L = gpu
    specs = [spec_of(first), spec_of(NAMES[(NAMES.index(first) + 1) % len(NAMES)])]
    handles = [s.create(L, False) for s in specs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rows = [130, 70, 130, 5]
    alone = [[outputs(call(L, s, "decode_batch", h, r, r, True, inputs=inputs_of(r, seed=r))) for r in rows] for s, h in zip(specs, handles)]
    for k, s in enumerate(specs):
        same(alone[k][0], s.model["decode_batch"](inputs_of(130, seed=130)), f"{s.name} alone against the model")
    pending = []
    for turn, r in enumerate(rows):
        for k, (s, h) in enumerate(zip(specs, handles)):
            stream = streams[(turn + k) % 2]
            pending.append((k, turn, call(L, s, "decode_batch", h, r, r, True, stream=stream.cuda_stream, inputs=inputs_of(r, seed=r))))
    torch.cuda.synchronize()
    for k, turn, result in pending:
        same(outputs(result), alone[k][turn], f"{specs[k].name}, turn {turn}")
    for s, h in zip(specs, handles):
        destroy(L, s, h)


# ---- the legs of a relay create ---------------------------------------------------------------------------------------------------

def _relay_create(L, name, legs=2, gammas=GAMMAS, leg_iters=(3, 2), stop_after=STOP_AFTER, alpha=0.0, prior0=None):
    from ldpcdecoders_jl_amd._host import _pattern_of, css_pattern
    import ldpcdecoders_jl_amd as ldpc

    g = None if gammas is None else np.ascontiguousarray(gammas, dtype=F)
    li = None if leg_iters is None else np.array(leg_iters, dtype=np.int32)
    gp, lp = (None if g is None else g.ctypes.data), (None if li is None else li.ctypes.data)
    h = ctypes.c_void_p()
    if name == "relay":
        o = ldpc._capi.RelayOptions()
        o.device, o.stop_after, o.alpha = -1, stop_after, alpha
        colptr, rowval = _csc(H)
        llr = LLR.copy() if prior0 is None else np.concatenate([[prior0], LLR[1:]]).astype(F)
        st = L.ldpc_relay_create(S, N, len(rowval), colptr.ctypes.data, rowval.ctypes.data, llr.ctypes.data, legs, gp, lp, ctypes.byref(o), ctypes.byref(h))
    else:
        o = ldpc._capi.PauliRelayOptions()
        o.device, o.stop_after, o.alpha = -1, stop_after, alpha
        px, pz = css_pattern(_pattern_of(HX)), css_pattern(_pattern_of(HZ))
        p = PRIORS.copy()
        if prior0 is not None:
            p[1, 0] = prior0
        st = L.ldpc_pauli_relay_create(N, ctypes.byref(px), ctypes.byref(pz), p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, legs, gp, lp,
                                       ctypes.byref(o), ctypes.byref(h))
    assert st != OK and not h.value
    return st, L.ldpc_last_error().decode()


@pytest.mark.parametrize("name", ["relay", "pauli_relay"])
def test_the_texts_of_a_relay_create_and_their_order(ldpc, gpu, name):
    """Every text of the checks of the legs, and where they stand among the other checks of a create: the arguments of the
    legs before the options, stop_after and the iterations after them, the priors next, the memory strengths last."""
    bad_gamma = GAMMAS.copy()
    bad_gamma[1, 2] = 1.0
    prior = "channel_llr[0] is not finite" if name == "relay" else "prior_y[0] is not finite"
    for change, text in ((dict(legs=0), "legs must be >= 1"),
                         (dict(legs=2 ** 31), "legs must fit int32"),
                         (dict(gammas=None), "gammas is NULL"),
                         (dict(leg_iters=None), "leg_iters is NULL"),
                         (dict(stop_after=-1), "stop_after must be >= 1 (0 = default 1)"),
                         (dict(leg_iters=(3, -1)), "leg_iters[1] is negative"),
                         (dict(leg_iters=(2 ** 31 - 1, 1)), "the sum of leg_iters exceeds INT32_MAX"),
                         (dict(gammas=bad_gamma), "gammas[1][2] must be finite and lie in (-1, 1)"),
                         (dict(legs=0, gammas=None), "legs must be >= 1"),
                         (dict(gammas=None, leg_iters=None), "gammas is NULL"),
                         (dict(leg_iters=None, alpha=1.5), "leg_iters is NULL"),
                         (dict(alpha=1.5, stop_after=-1), "alpha must lie in (0, 1]"),
                         (dict(stop_after=-1, leg_iters=(3, -1)), "stop_after must be >= 1 (0 = default 1)"),
                         (dict(leg_iters=(3, -1), prior0=np.inf), "leg_iters[1] is negative"),
                         (dict(prior0=np.nan, gammas=bad_gamma), prior)):
        assert _relay_create(gpu, name, **change) == (INVALID, text), (name, change)
