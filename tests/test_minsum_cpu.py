"""Min-sum decoder without a GPU: the numpy model of the rule (tests/minsum_model.py) on properties that follow from the
rule alone, the argument validation of ldpc_minsum_create (which answers before any device work), the Python
constructor's own refusals, and the `bp_decoder=` keyword of BeliefPropagationOSDDecoder at its default."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from minsum_model import MinSumModel, llr_of_probs

INVALID, NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def bb72():
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    H = sp.csc_matrix(np.asarray(Hx) != 0)
    assert H.shape == (36, 72) and set(np.diff(H.indptr)) == {3} and set(np.diff(sp.csr_matrix(H).indptr)) == {6}
    return H


def _syn(H, e):
    return ldpc.codes.syndromes_of(H, e)


def test_model_returns_every_weight_one_error(bb72):
    m = MinSumModel(bb72, llr_of_probs(np.full(72, 0.03)), 30, alpha=0.75)
    e = np.eye(72, dtype=np.uint8)
    err, conv, its, L = m.decode(_syn(bb72, e))
    assert np.array_equal(err, e) and conv.all() and its.min() >= 1 and its.max() <= 30
    assert L.dtype == np.float32 and np.array_equal(err, (L <= 0).astype(np.uint8))


def test_model_column_does_not_depend_on_its_neighbours(bb72):
    m = MinSumModel(bb72, llr_of_probs(np.full(72, 0.03)), 30)
    syn = _syn(bb72, ldpc.codes.random_errors(72, 40, 0.06, seed=5))
    err, conv, its, L = m.decode(syn)
    assert 0 < conv.sum() < 40   # stopped columns sit next to running ones: the freeze is exercised
    for c in (0, 7, 39):
        e1, c1, i1, L1 = m.decode(syn[c:c + 1])
        assert np.array_equal(e1[0], err[c]) and c1[0] == conv[c] and i1[0] == its[c]
        assert np.array_equal(L1[0].view(np.int32), L[c].view(np.int32))
    perm = np.random.default_rng(1).permutation(40)
    e2, c2, i2, L2 = m.decode(syn[perm])
    assert np.array_equal(e2, err[perm]) and np.array_equal(i2, its[perm]) and np.array_equal(L2.view(np.int32), L[perm].view(np.int32))


def test_model_max_iters_zero(bb72):
    err, conv, its, L = MinSumModel(bb72, llr_of_probs(np.full(72, 0.03)), 0).decode(np.ones((3, 36), dtype=np.uint8))
    assert not err.any() and not conv.any() and not its.any() and not L.any() and L.dtype == np.float32


def test_model_clip_is_exercised(bb72):
    """At p = 0.06, alpha = 1 the posteriors grow past 8 (magnitudes of 35-42 were seen), so clip = 8 changes a column."""
    syn = _syn(bb72, ldpc.codes.random_errors(72, 64, 0.06, seed=9))
    prior = llr_of_probs(np.full(72, 0.06))
    a = MinSumModel(bb72, prior, 50, alpha=1.0, clip=8.0).decode(syn)
    b = MinSumModel(bb72, prior, 50, alpha=1.0, clip=1e6).decode(syn)
    assert np.abs(b[3]).max() > 8.0
    assert any(not np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))
    assert (a[3].view(np.int32) != b[3].view(np.int32)).any(axis=1).sum() >= 1


def test_model_hand_checked_cases():
    # one check over two bits, syndrome 1, priors 2 and 1, alpha 0.5: b = (2, 1), m1 = 1 at a = 1, m2 = 2, par = 1:
    # c = (-0.5 * 1, -0.5 * 2) = (-0.5, -1); L = (1.5, 0): err = (0, 1) (L <= 0), matched in iteration 1
    H = np.array([[1, 1]], dtype=np.uint8)
    err, conv, its, L = MinSumModel(H, [2.0, 1.0], 5, alpha=0.5).decode(np.array([[1]]))
    assert err.tolist() == [[0, 1]] and conv[0] == 1 and its[0] == 1 and L.tolist() == [[1.5, 0.0]]
    # every magnitude at the clip: a stays "none", both messages carry alpha * clip
    err, conv, its, L = MinSumModel(H, [9.0, 9.0], 1, alpha=0.5, clip=4.0).decode(np.array([[0]]))
    assert L.tolist() == [[11.0, 11.0]] and conv[0] == 1
    # an empty check is matched only by a 0 entry; an isolated bit with a negative prior is an error from the prior alone
    H = np.array([[0, 0], [1, 0]], dtype=np.uint8)
    m = MinSumModel(H, [3.0, -1.0], 2)
    err, conv, its, L = m.decode(np.array([[0, 0], [1, 0], [2, 0]]))
    assert err.tolist() == [[0, 1]] * 3 and conv.tolist() == [1, 0, 0] and its.tolist() == [1, 2, 2]
    # a zero magnitude with the sign set is -0: +0 + -0 = +0, and L <= 0 holds for both zeros
    H = np.array([[1, 1]], dtype=np.uint8)
    err, conv, its, L = MinSumModel(H, [0.0, 0.0], 1, alpha=1.0).decode(np.array([[1]]))
    assert not L.any() and not np.signbit(L).any() and err.tolist() == [[1, 1]] and conv[0] == 0


# ---- ldpc_minsum_create validates before it looks for a device ------------------------------------------------------

def _create(colptr, rowval, s, n, llr, max_iters=10, alpha=None, clip=None, variant=0, opts=True):
    L = ldpc._capi.lib()
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    llr = np.asarray(llr, dtype=np.float32)
    o = ldpc._capi.MinSumOptions()
    o.device = -1
    if alpha is not None:
        o.alpha = alpha
    if clip is not None:
        o.clip = clip
    o.kernel_variant = variant
    h = ctypes.c_void_p()
    st = L.ldpc_minsum_create(s, n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data, llr.ctypes.data, max_iters,
                              ctypes.byref(o) if opts else None, ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    if st == 0:
        assert L.ldpc_minsum_kernel(h) in (1, 2)
        L.ldpc_minsum_destroy(h)
    else:
        assert not h.value
    return st, msg


GOOD = dict(colptr=[0, 2, 3, 5], rowval=[0, 1, 1, 0, 2], s=3, n=3, llr=[1.0, -2.0, 3.0])


@pytest.mark.parametrize("change, word", [
    (dict(llr=[1.0, np.nan, 3.0]), "channel_llr[1]"),
    (dict(llr=[np.inf, 2.0, 3.0]), "channel_llr[0]"),
    (dict(llr=[1.0, 2.0, -np.inf]), "channel_llr[2]"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=-0.25), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(clip=float("inf")), "clip"),
    (dict(clip=-1.0), "clip"),
    (dict(clip=float("nan")), "clip"),
    (dict(variant=3), "kernel_variant"),
    (dict(max_iters=-1), "max_iters"),
    (dict(rowval=[1, 0, 1, 0, 2]), "ascending"),       # unsorted CSC
    (dict(rowval=[0, 1, 1, 0, 3]), "rowval"),          # a row out of range
    (dict(colptr=[0, 2, 3, 4]), "colptr"),
])
def test_create_rejects_bad_arguments_before_any_device_work(change, word):
    st, msg = _create(**{**GOOD, **change})
    assert st == INVALID and word in msg, (st, msg)


def test_create_zero_alpha_and_clip_select_the_defaults():
    """A zeroed options struct means defaults (include/ldpc_mi355x.h): validation passes, and what answers then is the
    device lookup -- LDPC_OK with a GPU, LDPC_ERR_NO_DEVICE without.  From Python a zero is refused instead (below)."""
    for kw in (dict(), dict(alpha=0.0, clip=0.0), dict(opts=False)):
        st, msg = _create(**{**GOOD, **kw})
        assert st in (0, NO_DEVICE), (st, msg)
    L = ldpc._capi.lib()
    assert L.ldpc_minsum_kernel(None) == 0 and L.ldpc_minsum_destroy(None) == 0
    assert L.ldpc_minsum_decode_batch(None, 1, None, None, None, None, None) == INVALID
    assert L.ldpc_minsum_decode_batch_device(None, 1, None, None, None, None, None, None) == INVALID
    assert ctypes.sizeof(ldpc._capi.MinSumOptions) == 64


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(clip=0.0), dict(alpha=1.5), dict(clip=float("inf")),
                                dict(channel_llr=[1.0, float("nan"), 2.0], per=None)])
def test_constructor_reports_invalid_argument_with_a_message(kw):
    H = sp.csc_matrix((np.ones(5), GOOD["rowval"], GOOD["colptr"]), shape=(3, 3))
    args = {"per": 0.05, **kw}
    with pytest.raises(ldpc.LdpcError) as e:
        ldpc.MinSumDecoder(H, args.pop("per"), 10, **args)
    assert e.value.status == INVALID and e.value.message


def test_constructor_takes_exactly_one_prior_and_probabilities_inside_the_unit_interval():
    H = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    for kw in (dict(per=0.1, channel_probs=[0.1] * 3), dict(per=0.1, channel_llr=[1.0] * 3),
               dict(channel_probs=[0.1] * 3, channel_llr=[1.0] * 3), dict()):
        with pytest.raises(TypeError):
            ldpc.MinSumDecoder(H, kw.pop("per", None), 10, **kw)
    for probs in ([0.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, float("nan")], [0.1, -0.2, 0.1]):
        with pytest.raises(ValueError):
            ldpc.MinSumDecoder(H, None, 10, channel_probs=probs)
    for per in (0.0, 1.0):
        with pytest.raises(ValueError):
            ldpc.MinSumDecoder(H, per, 10)
    with pytest.raises(ValueError):
        ldpc.MinSumDecoder(H, None, 10, channel_llr=[1.0, 2.0])   # one prior per bit
    # the package's own prior equals the model's, bit for bit
    from ldpcdecoders_jl_amd.minsum import llr_of_probs as pkg_llr
    p = np.random.default_rng(3).uniform(1e-4, 0.9, 100)
    assert np.array_equal(pkg_llr(p).view(np.int32), llr_of_probs(p).view(np.int32))


def test_bposd_default_builds_the_sum_product_decoder_as_before(monkeypatch):
    """bp_decoder=None: BeliefPropagationDecoder(H, per, max_iters, llr_exact=True, **keywords), as before the keyword."""
    import ldpcdecoders_jl_amd.osd as osd

    calls = []

    class Recorder:
        def __init__(self, *a, **kw):
            calls.append((a, kw))
            self.sparse_H = sp.csc_matrix(a[0])

    monkeypatch.setattr(osd, "BeliefPropagationDecoder", Recorder)
    H = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    d = osd.BeliefPropagationOSDDecoder(H, 0.05, 7, osd_order=2)
    assert type(d.bp_decoder) is Recorder and d.osd_order == 2 and d.osd == "host"
    d2 = osd.BeliefPropagationOSDDecoder(H, 0.05, 7, bp_decoder=None, kernel_variant=2, llr_exact=False)
    assert [(a[1:], kw) for a, kw in calls] == [((0.05, 7), {"llr_exact": True}),
                                                ((0.05, 7), {"llr_exact": False, "kernel_variant": 2})]
    assert all(a[0] is H for a, _ in calls)
    # a given object is used as it is; H is checked against it, per and max_iters are ignored
    given = Recorder(H)
    d3 = osd.BeliefPropagationOSDDecoder(H, osd_order=1, bp_decoder=given)
    assert d3.bp_decoder is given and len(calls) == 3
    with pytest.raises(ValueError):
        osd.BeliefPropagationOSDDecoder(np.array([[1, 0, 1], [0, 1, 1]]), bp_decoder=given)
    with pytest.raises(TypeError):
        osd.BeliefPropagationOSDDecoder(H, bp_decoder=given, llr_exact=True)
    assert d2.bp_decoder is not given
    # without bp_decoder=, per and max_iters are required as before
    for args in ((H,), (H, 0.05)):
        with pytest.raises(TypeError):
            osd.BeliefPropagationOSDDecoder(*args, osd_order=1)
