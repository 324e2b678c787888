"""Relay min-sum decoder without a GPU: the numpy model of the rule (tests/relay_model.py) on properties that follow from
the rule alone, the argument validation of ldpc_relay_create (which answers before any device work), the Python
constructor's own refusals, and the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from minsum_model import MinSumModel, llr_of_probs
from relay_model import RelayModel, weights_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = 1, 2
NEW_SYMBOLS = ("ldpc_relay_create", "ldpc_relay_destroy", "ldpc_relay_kernel", "ldpc_relay_decode_batch",
               "ldpc_relay_decode_batch_device")


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def bb72():
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx) != 0)


def _gammas(legs, n, seed=5):
    g = np.empty((legs, n), dtype=np.float32)
    g[0] = 0.125
    g[1:] = np.random.default_rng(seed).uniform(-0.24, 0.66, size=(legs - 1, n)).astype(np.float32)
    return g


@pytest.mark.parametrize("per", [0.03, 0.06])
def test_model_with_gamma_zero_and_one_leg_is_the_minsum_model(bb72, per):
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 100, per, seed=3))
    prior = llr_of_probs(np.full(72, per))
    err, conv, its, found, M = RelayModel(bb72, prior, np.zeros((1, 72)), [30]).decode(syn)
    merr, mconv, mits, mL = MinSumModel(bb72, prior, 30).decode(syn)
    assert 0 < mconv.sum() < 100 or per == 0.03
    assert np.array_equal(err, merr) and np.array_equal(conv, mconv) and np.array_equal(its, mits)
    assert np.array_equal(M.view(np.int32), mL.view(np.int32)) and np.array_equal(found, mconv.astype(np.int32))


def test_model_column_does_not_depend_on_its_neighbours(bb72):
    """Short legs, so that one batch holds columns that stop in leg 0, columns that stop later and columns that never do."""
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 60, 0.06, seed=3))
    m = RelayModel(bb72, llr_of_probs(np.full(72, 0.06)), _gammas(3, 72), [6, 4, 4], stop_after=2)
    err, conv, its, found, M = full = m.decode(syn)
    assert (conv == 0).any() and ((conv == 1) & (its <= 6)).any() and ((conv == 1) & (its > 6)).any()
    assert len(set(found.tolist())) == 3
    picks = [int(np.nonzero(conv == 0)[0][0]), int(np.nonzero((conv == 1) & (its <= 6))[0][0]), int(np.nonzero(its > 6)[0][-1]), 59]
    for c in picks:
        assert _same(m.decode(syn[c:c + 1]), tuple(x[c:c + 1] for x in full))
    perm = np.random.default_rng(1).permutation(60)
    assert _same(m.decode(syn[perm]), tuple(x[perm] for x in full))


def test_model_hand_checked_case_with_memory():
    """One check over two bits, syndrome 0, priors (2, -1), alpha 0.5, gamma 0.5: g0 = (1, -0.5), X = g0 + 0.5 M = (2, -1).
    t = 1: b = (2, -1), m1 = 1 at a = 1, m2 = 2, par = 1: c = (-0.5, +1); Lambda = (2, -1), M = (1.5, 0);
           Lambda' = (1.75, -0.5), X = (1.25, 0.5); err = (0, 1): not matched.
    t = 2: b = X - c = (1.75, -0.5), m1 = 0.5 at a = 1, m2 = 1.75, par = 1: c = (-0.25, +0.875); Lambda = (1.75, -0.5),
           M = (1.5, 0.375); Lambda' = (1.75, -0.3125), X = (1.5, 0.5625); err = (0, 0): matched."""
    trace = []
    m = RelayModel(np.array([[1, 1]], dtype=np.uint8), [2.0, -1.0], [[0.5, 0.5]], [5], alpha=0.5)
    err, conv, its, found, M = m.decode(np.array([[0]]), trace=trace)
    assert m.g0.tolist() == [[1.0, -0.5]]
    assert [(tr[2].tolist(), tr[3].tolist()) for tr in trace] == [([[1.5, 0.0]], [[1.25, 0.5]]), ([[1.5, 0.375]], [[1.5, 0.5625]])]
    assert err.tolist() == [[0, 0]] and conv[0] == 1 and its[0] == 2 and found[0] == 1 and M.tolist() == [[1.5, 0.375]]
    # without memory the same input is the min-sum model's
    plain = RelayModel(np.array([[1, 1]], dtype=np.uint8), [2.0, -1.0], [[0.0, 0.0]], [5], alpha=0.5).decode(np.array([[0]]))
    ms = MinSumModel(np.array([[1, 1]], dtype=np.uint8), [2.0, -1.0], 5, alpha=0.5).decode(np.array([[0]]))
    assert np.array_equal(plain[4].view(np.int32), ms[3].view(np.int32)) and plain[2][0] == ms[2][0]


def test_model_a_later_lighter_solution_replaces_best(bb72):
    """Per-bit priors: with stop_after = 3 some column meets a later solution of strictly lower weight, which is returned."""
    rng = np.random.default_rng(17)
    probs = rng.uniform(0.01, 0.12, 72)
    prior = llr_of_probs(probs)
    syn = ldpc.codes.syndromes_of(bb72, (rng.random((120, 72)) < probs[None, :]).astype(np.uint8))
    legs = [20, 12, 12, 12, 12, 12]
    trace = []
    m3 = RelayModel(bb72, prior, _gammas(6, 72), legs, stop_after=3)
    err3, conv3, _, found3, _ = m3.decode(syn, trace=trace)
    err1, conv1, _, _, _ = RelayModel(bb72, prior, _gammas(6, 72), legs, stop_after=1).decode(syn)
    q = weights_of(prior)
    hits = {}
    for _, _, M, _, w, hit in trace:
        for b in np.nonzero(hit)[0]:
            assert w[b] == int(((M[b] <= 0) * q).sum())
            hits.setdefault(int(b), []).append((int(w[b]), (M[b] <= 0).astype(np.uint8)))
    replaced = [b for b, h in hits.items() if min(x[0] for x in h[1:] or h) < h[0][0]]
    assert replaced
    for b, h in hits.items():
        first_lightest = min(range(len(h)), key=lambda k: (h[k][0], k))
        assert np.array_equal(err3[b], h[first_lightest][1]) and found3[b] == len(h) <= 3
        assert np.array_equal(err1[b], h[0][1])
    for b in replaced:
        assert (err3[b] * q).sum() < (err1[b] * q).sum() and (err3[b] != err1[b]).any()
    assert np.array_equal(conv3, conv1)
    assert np.array_equal(ldpc.codes.syndromes_of(bb72, err3[conv3 == 1]), syn[conv3 == 1])


TIE = dict(H=np.array([[1, 1, 0, 0], [0, 1, 1, 1]], dtype=np.uint8), prior=[1.0, 1.0, 1.0, 1.0],
           gammas=[[0.75, -0.625, 0.75, -0.375], [-0.125, 0.625, -0.125, 0.125], [-0.875, 0.5, 0.125, -0.25]],
           leg_iters=[3, 3, 3], syn=np.array([[0, 1]], dtype=np.uint8))


def test_model_a_tie_keeps_the_earlier_solution():
    """Equal priors: (0, 0, 1, 0) is found first, then (0, 0, 0, 1) of the same weight: the first one stays."""
    trace = []
    m = RelayModel(TIE["H"], TIE["prior"], TIE["gammas"], TIE["leg_iters"], alpha=1.0, stop_after=3)
    err, conv, its, found, M = m.decode(TIE["syn"], trace=trace)
    hits = [(int(w[0]), (Mt[0] <= 0).astype(int).tolist()) for _, _, Mt, _, w, hit in trace if hit[0]]
    assert [h[1] for h in hits[:2]] == [[0, 0, 1, 0], [0, 0, 0, 1]] and hits[0][0] == hits[1][0] == 65536
    assert err.tolist() == [[0, 0, 1, 0]] and found[0] == len(hits) == 3 and conv[0] == 1
    assert (M[0] <= 0).astype(int).tolist() != err[0].tolist()   # the LLRs are those of the LAST solution, not of best


def test_weights_clamp_large_priors_and_round_subnormal_ones_to_zero():
    q = weights_of(np.array([1.0, -0.5, 3.0e7, -5.0e7, 1e-40, -1e-40, 2.0 ** 24, 1.5 * 2.0 ** -17, 2.5 * 2.0 ** -17, 0.0], dtype=np.float32))
    assert q.dtype == np.int64
    assert q.tolist() == [65536, -32768, 2 ** 40, -2 ** 40, 0, 0, 2 ** 40, 1, 1, 0]      # 0.75 -> 1, 1.25 -> 1: rint
    assert weights_of(np.array([0.5 * 2.0 ** -16, 1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16], dtype=np.float32)).tolist() == [0, 2, 2]   # ties to even
    assert weights_of(llr_of_probs([0.03]))[0] == int(np.rint(float(llr_of_probs([0.03])[0]) * 65536.0))


def test_model_a_leg_of_zero_iterations_is_skipped_and_all_zero_legs_give_zeros(bb72):
    syn = ldpc.codes.syndromes_of(bb72, ldpc.codes.random_errors(72, 40, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    g = _gammas(4, 72)
    with_gap = RelayModel(bb72, prior, g, [5, 0, 4, 4], stop_after=2).decode(syn)
    without = RelayModel(bb72, prior, g[[0, 2, 3]], [5, 4, 4], stop_after=2).decode(syn)
    assert _same(with_gap, without) and (with_gap[2] > 5).any()
    assert not _same(with_gap, RelayModel(bb72, prior, g[[0, 1, 3]], [5, 4, 4], stop_after=2).decode(syn))
    err, conv, its, found, M = RelayModel(bb72, prior, g, [0, 0, 0, 0]).decode(syn)
    assert not err.any() and not conv.any() and not its.any() and not found.any() and not M.view(np.int32).any()
    assert M.dtype == np.float32 and its.dtype == np.int32 and found.dtype == np.int32


# ---- the new symbols; ldpc_relay_create validates before it looks for a device --------------------------------------

@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_declared_and_listed(experiments):
    lib = ldpc._capi.lib(experiments)
    hdr = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    jl = open(os.path.join(ROOT, "ldpcdecoders.jl_amd", "julia", "LDPCDecodersMI355X.jl")).read()
    for name in NEW_SYMBOLS:
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("ldpc_relay_create", "ldpc_relay_destroy", "ldpc_relay_decode_batch"):
        assert ":%s" % name in jl, name
    assert lib.ldpc_abi_version() == 4   # added by symbol
    assert ctypes.sizeof(ldpc._capi.RelayOptions) == 64
    assert "RelayMinSumDecoder" in ldpc.__all__ and ldpc.RelayMinSumDecoder.__mro__[1] is ldpc.AbstractDecoder
    for method in ("decode_batch_host", "decode_batch_device", "decode_", "batchdecode_", "info", "close"):
        assert callable(getattr(ldpc.RelayMinSumDecoder, method))


def _create(colptr, rowval, s, n, llr, gammas, leg_iters, legs=None, alpha=None, clip=None, variant=0, stop_after=0,
            opts=True, null=()):
    L = ldpc._capi.lib()
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    llr = np.asarray(llr, dtype=np.float32)
    gammas = np.ascontiguousarray(gammas, dtype=np.float32)
    leg_iters = np.asarray(leg_iters, dtype=np.int32)
    o = ldpc._capi.RelayOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    o.kernel_variant, o.stop_after = variant, stop_after
    h = ctypes.c_void_p()
    st = L.ldpc_relay_create(s, n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                             None if "llr" in null else llr.ctypes.data, len(leg_iters) if legs is None else legs,
                             None if "gammas" in null else gammas.ctypes.data,
                             None if "leg_iters" in null else leg_iters.ctypes.data,
                             ctypes.byref(o) if opts else None, ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_relay_kernel(h) in (1, 2)
        L.ldpc_relay_destroy(h)
    else:
        assert not h.value
    return st, msg


GOOD = dict(colptr=[0, 2, 3, 5], rowval=[0, 1, 1, 0, 2], s=3, n=3, llr=[1.0, -2.0, 3.0],
            gammas=[[0.125, 0.125, 0.125], [-0.2, 0.5, 0.0]], leg_iters=[10, 5])


@pytest.mark.parametrize("change, word", [
    (dict(null=("llr",)), "channel_llr is NULL"),
    (dict(null=("gammas",)), "gammas is NULL"),
    (dict(null=("leg_iters",)), "leg_iters is NULL"),
    (dict(llr=[1.0, np.nan, 3.0]), "channel_llr[1]"),
    (dict(llr=[np.inf, 2.0, 3.0]), "channel_llr[0]"),
    (dict(llr=[1.0, 2.0, -np.inf]), "channel_llr[2]"),
    (dict(gammas=[[0.1, 0.1, 0.1], [0.1, np.nan, 0.1]]), "gammas[1][1]"),
    (dict(gammas=[[0.1, 0.1, np.inf], [0.1, 0.1, 0.1]]), "gammas[0][2]"),
    (dict(gammas=[[1.0, 0.1, 0.1], [0.1, 0.1, 0.1]]), "gammas[0][0]"),
    (dict(gammas=[[0.1, 0.1, 0.1], [0.1, 0.1, -1.0]]), "gammas[1][2]"),
    (dict(gammas=[[0.1, 0.1, 0.1], [-1.5, 0.1, 0.1]]), "gammas[1][0]"),
    (dict(legs=0), "legs"),
    (dict(legs=-2), "legs"),
    (dict(leg_iters=[10, -1]), "leg_iters[1]"),
    (dict(leg_iters=[2 ** 31 - 1, 1]), "sum of leg_iters"),
    (dict(stop_after=-1), "stop_after"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=-0.25), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(clip=float("inf")), "clip"),
    (dict(clip=-1.0), "clip"),
    (dict(clip=float("nan")), "clip"),
    (dict(variant=3), "kernel_variant"),
    (dict(variant=-1), "kernel_variant"),
    (dict(rowval=[1, 0, 1, 0, 2]), "ascending"),       # unsorted CSC
    (dict(rowval=[0, 1, 1, 0, 3]), "rowval"),          # a row out of range
    (dict(colptr=[0, 2, 3, 4]), "colptr"),
])
def test_create_rejects_bad_arguments_before_any_device_work(change, word):
    st, msg = _create(**{**GOOD, **change})
    assert st == INVALID and word in msg, (st, msg)


def test_create_accepts_the_edges_of_the_ranges_and_a_zeroed_options_struct():
    """Validation passes, and what answers then is the device lookup: LDPC_OK with a GPU, LDPC_ERR_NO_DEVICE without."""
    edge = np.nextafter(np.float32(1.0), np.float32(0.0))
    for kw in (dict(), dict(alpha=0.0, clip=0.0, stop_after=0), dict(opts=False), dict(stop_after=5),
               dict(gammas=[[edge, -edge, 0.0], [0.0, 0.0, 0.0]]), dict(leg_iters=[0, 0]), dict(leg_iters=[2 ** 31 - 2, 1])):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (0, NO_DEVICE), (st, msg)
        if ldpc._capi.lib().ldpc_device_count() == 0:
            assert st == NO_DEVICE
    L = ldpc._capi.lib()
    assert L.ldpc_relay_kernel(None) == 0 and L.ldpc_relay_destroy(None) == 0
    assert L.ldpc_relay_decode_batch(None, 1, None, None, None, None, None, None) == INVALID
    assert L.ldpc_relay_decode_batch_device(None, 1, None, None, None, None, None, None, None) == INVALID


# ---- the Python constructor's own refusals ---------------------------------------------------------------------------

H3 = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)


def test_constructor_takes_exactly_one_prior():
    for kw in (dict(per=0.1, channel_probs=[0.1] * 3), dict(per=0.1, channel_llr=[1.0] * 3),
               dict(channel_probs=[0.1] * 3, channel_llr=[1.0] * 3), dict()):
        with pytest.raises(TypeError):
            ldpc.RelayMinSumDecoder(H3, kw.pop("per", None), 10, **kw)
    for probs in ([0.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, float("nan")]):
        with pytest.raises(ValueError):
            ldpc.RelayMinSumDecoder(H3, None, 10, channel_probs=probs)
    with pytest.raises(ValueError):
        ldpc.RelayMinSumDecoder(H3, None, 10, channel_llr=[1.0, 2.0])   # one prior per bit


def test_constructor_checks_types_shapes_and_ranges():
    for kw in (dict(max_iters=10.0), dict(max_iters=True), dict(legs=2.0), dict(leg_iters=3.5), dict(stop_after=1.0), dict(per=1)):
        args = {"per": 0.05, "max_iters": 10, **kw}
        with pytest.raises(TypeError):
            ldpc.RelayMinSumDecoder(H3, args.pop("per"), args.pop("max_iters"), **args)
    for kw in (dict(legs=0), dict(stop_after=0), dict(leg_iters=-1), dict(max_iters=-1), dict(gammas=np.zeros((2, 3))),   # (legs = 9)
               dict(legs=2, gammas=np.zeros((2, 4))), dict(gamma0=1.0), dict(gamma_range=(-1.0, 0.5)), dict(gamma_range=(0.5, 0.2))):
        args = {"max_iters": 10, **kw}
        with pytest.raises(ValueError):
            ldpc.RelayMinSumDecoder(H3, 0.05, args.pop("max_iters"), **args)


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")),
                                dict(legs=2, gammas=[[0.1, 0.1, 0.1], [0.1, 1.0, 0.1]]),
                                dict(legs=1, gammas=[[0.1, float("nan"), 0.1]]),
                                dict(channel_llr=[1.0, float("nan"), 2.0], per=None), dict(kernel_variant=3)])
def test_constructor_reports_invalid_argument_with_a_message(kw):
    args = {"per": 0.05, **kw}
    with pytest.raises(ldpc.LdpcError) as e:
        ldpc.RelayMinSumDecoder(H3, args.pop("per"), 10, **args)
    assert e.value.status == INVALID and e.value.message


def test_constructor_hands_over_the_arrays_it_documents(monkeypatch):
    """.gammas and .leg_iters as documented: leg 0 is gamma0, legs 1... are uniform in gamma_range from the seed; without
    a device the library answers LDPC_ERR_NO_DEVICE after it has accepted them, so the arrays are read off a stub."""
    seen = {}

    class Stub:
        def __getattr__(self, name):
            def call(*a):
                seen[name] = a
                return 0
            return call

    monkeypatch.setattr(ldpc._capi, "lib_for", lambda *_: Stub())
    d = ldpc.RelayMinSumDecoder(H3, 0.05, 30, legs=4, leg_iters=7, seed=11, stop_after=2, device=0)
    want = np.random.default_rng(11).uniform(-0.24, 0.66, size=(3, 3)).astype(np.float32)
    assert d.gammas.dtype == np.float32 and d.gammas.shape == (4, 3) and (d.gammas[0] == np.float32(0.125)).all()
    assert np.array_equal(d.gammas[1:], want) and d.leg_iters.dtype == np.int32 and d.leg_iters.tolist() == [30, 7, 7, 7]
    assert np.array_equal(d.channel_llr.view(np.int32), llr_of_probs(np.full(3, 0.05)).view(np.int32))
    a = seen["ldpc_relay_create"]
    assert a[:3] == (2, 3, 4) and a[6] == 4 and a[5] == d.channel_llr.ctypes.data and a[7] == d.gammas.ctypes.data and a[8] == d.leg_iters.ctypes.data
    g = np.array([[0.5, -0.5, 0.0]], dtype=np.float64)
    d = ldpc.RelayMinSumDecoder(H3, None, 5, channel_llr=[1.0, 2.0, 3.0], legs=1, gammas=g, device=0)
    assert np.array_equal(d.gammas, g.astype(np.float32)) and d.leg_iters.tolist() == [5] and d.per is None
