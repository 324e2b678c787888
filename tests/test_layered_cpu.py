"""The layered min-sum schedule without a GPU: the numpy model of THE LAYERED RULE (tests/layered_model.py) against hand
calculations and its own invariants, against the flooding model (tests/minsum_model.py) on the two cases the schedule was
proposed with, and the refusals of ldpc_minsum_create / MinSumDecoder that answer before any device work."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from layered_model import LayeredMinSumModel, layers_of
from minsum_model import MinSumModel, llr_of_probs

F = np.float32
INVALID, NO_DEVICE = 1, 2


# ---- the model against hand calculations -----------------------------------------------------------------------------

def test_three_checks_by_hand():
    """H = [[1 1 0] [0 1 1] [1 0 1]], prior (2, -1, 3), alpha 0.5, syndrome (1, 0, 0).  Every check meets the others: one
    check per layer, K = 3.  One iteration, every value exact in binary32:
      check 0 (bits 0, 1; entry 1): b = (2, -1); m1 = 1 (a = 1), m2 = 2; par = 1 ^ 1 = 0; c = (+0.5, -1): the sign is
        par ^ neg = (0, 1), the value alpha * (m1, m2) = (0.5, 1);  L = (2.5, -2, 3)
      check 1 (bits 1, 2; entry 0): b = (-2, 3); m1 = 2 (a = 0), m2 = 3; par = 1; c = (+1.5, -1): signs (1 ^ 1, 1 ^ 0),
        values alpha * (m2, m1);  L = (2.5, -0.5, 2)
      check 2 (bits 0, 2; entry 0): b = (2.5, 2); m1 = 2 (a = 1), m2 = 2.5; par = 0; c = (+1, +1.25);  L = (3.5, -0.5, 3.25)
    err = (0, 1, 0): H err = (1, 1, 0) != syndrome -- not converged after one iteration."""
    H = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.uint8)
    assert layers_of(H)[0].tolist() == [0, 1, 2] and layers_of(H)[1] == 3
    m = LayeredMinSumModel(H, [2.0, -1.0, 3.0], 1, alpha=0.5)
    assert m.layers == [[0], [1], [2]]
    err, conv, its, L = m.decode(np.array([[1, 0, 0]]))
    assert L.tolist() == [[3.5, -0.5, 3.25]] and err.tolist() == [[0, 1, 0]] and conv.tolist() == [0] and its.tolist() == [1]
    # the flooding rule on the same input differs after one iteration: every check reads the priors
    #   c0 = (+0.5, -1), c1 = (+1.5, -0.5), c2 = (+1.5, +1); L = (2 + 0.5 + 1.5, -1 - 1 + 1.5, 3 - 0.5 + 1) = (4, -0.5, 3.5)
    assert MinSumModel(H, [2.0, -1.0, 3.0], 1, alpha=0.5).decode(np.array([[1, 0, 0]]))[3].tolist() == [[4.0, -0.5, 3.5]]
    # a second iteration, check 0: the own message comes off first: b = (3.5 - 0.5, -0.5 + 1) = (3, 0.5); m1 = 0.5 (a = 1),
    # m2 = 3; par = 1 ^ 0 = 1: c = (-0.25, -1.5); L = (2.75, -1, 3.25)
    one = LayeredMinSumModel(H, [2.0, -1.0, 3.0], 2, alpha=0.5, layers=[[0], [1], [2]])
    b = np.minimum(np.maximum(L[:, [0, 1]] - np.array([[0.5, -1.0]], dtype=F), F(-1e6)), F(1e6))
    assert b.tolist() == [[3.0, 0.5]] and one.decode(np.array([[1, 0, 0]]))[2].tolist() == [2]


def test_stop_clip_degree_zero_and_max_iters_zero():
    # a converged column stops at its iteration and keeps its L; an empty check is matched only by a 0 entry
    H = np.array([[1, 1, 0], [0, 0, 0]], dtype=np.uint8)
    m = LayeredMinSumModel(H, [1.0, 2.0, -4.0], 3, alpha=1.0)
    assert m.K == 1 and m.layer_of.tolist() == [0, -1]
    err, conv, its, L = m.decode(np.array([[0, 0], [1, 0], [0, 1]]))
    # column 0: b = (1, 2), par 0: c = (2, 1), L = (3, 3): converged at 1.  bit 2 (degree 0) keeps its prior
    assert L[0].tolist() == [3.0, 3.0, -4.0] and (conv[0], its[0]) == (1, 1) and err[0].tolist() == [0, 0, 1]
    # column 1: par 1: c = (-2, -1), L = (-1, 1): err (1, 0, 1) gives H err = (1, 0): converged at 1
    assert L[1].tolist() == [-1.0, 1.0, -4.0] and (conv[1], its[1]) == (1, 1)
    assert (conv[2], its[2]) == (0, 3)                                   # the empty check's entry is 1
    # the clamp: |b| <= clip before the minima
    err, conv, its, L = LayeredMinSumModel(np.array([[1, 1]]), [100.0, -50.0], 1, alpha=1.0, clip=8.0).decode(np.array([[0]]))
    assert L.tolist() == [[8.0 - 8.0, -8.0 + 8.0]]                        # b = (8, -8); par 1; c = (-8, +8)
    out = LayeredMinSumModel(H, [1.0, 2.0, -4.0], 0).decode(np.array([[0, 0], [1, 1]]))
    assert not out[0].any() and not out[1].any() and not out[2].any() and not out[3].view(np.int32).any()
    # -0: a zero magnitude with the sign set; b + -0 = b
    err, conv, its, L = LayeredMinSumModel(np.array([[1, 1]]), [0.0, 3.0], 1, alpha=1.0).decode(np.array([[1]]))
    assert L.tolist() == [[-3.0, 3.0]] and not np.signbit(L[0, 1])        # c = (-3, -0)


# ---- the two cases of the proposal ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def proposal_case(name):
    if name == "bb72":
        H = sp.csc_matrix(np.asarray(ldpc.codes.bivariate_bicycle_72_12_6()[0], dtype=np.uint8))
        n, B, rate = 72, 400, 0.06
    else:
        H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
        n, B, rate = 240, 200, 0.05
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, B, rate, seed=3))
    prior = llr_of_probs(np.full(n, rate))
    flood = MinSumModel(H, prior, 30).decode(syn)
    layered = LayeredMinSumModel(H, prior, 30).decode(syn)
    return H, prior, syn, flood, layered


@pytest.mark.parametrize("name", ["bb72", "240_8_4"])
def test_layered_converges_at_least_as_often_and_in_fewer_iterations(name):
    _, _, syn, flood, layered = proposal_case(name)
    both = (flood[1] == 1) & (layered[1] == 1)
    ratio = layered[2][both].mean() / flood[2][both].mean()
    print(f"{name}: converged {int(flood[1].sum())} -> {int(layered[1].sum())} of {len(syn)}, mean iterations "
          f"{flood[2][both].mean():.2f} -> {layered[2][both].mean():.2f} (ratio {ratio:.2f})")
    assert layered[1].sum() >= flood[1].sum()
    assert both.sum() > len(syn) // 2 and ratio < 0.7
    # every column it calls converged reproduces its syndrome
    H = proposal_case(name)[0]
    ok = layered[1] == 1
    assert np.array_equal(ldpc.codes.syndromes_of(H, layered[0][ok]), syn[ok])


def test_a_permutation_inside_a_layer_changes_no_bit():
    H, prior, syn, _, want = proposal_case("bb72")
    m = LayeredMinSumModel(H, prior, 30)
    assert m.K == 4 and all(len(ly) > 1 for ly in m.layers)
    rng = np.random.default_rng(5)
    shuffled = [list(rng.permutation(ly)) for ly in m.layers]
    assert shuffled != m.layers
    got = LayeredMinSumModel(H, prior, 30, layers=shuffled).decode(syn[:120])
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w[:120].view(np.uint8))
    # ... while another order of the LAYERS does change the result: the assignment is part of the rule
    other = LayeredMinSumModel(H, prior, 30, layers=m.layers[::-1]).decode(syn[:120])
    assert (other[3].view(np.int32) != want[3][:120].view(np.int32)).any()


def test_one_check_per_layer_is_the_serial_schedule():
    """With every check a layer of its own the model is the plain serial sweep in that order; on a graph whose first-fit
    layers are single checks (a chain) it equals the rule's own layering in every bit."""
    n = 9
    Hd = np.zeros((n - 1, n), dtype=np.uint8)
    for i in range(n - 1):
        Hd[i, i] = Hd[i, i + 1] = 1                       # a chain: check i meets check i - 1
    prior = llr_of_probs(np.linspace(0.02, 0.3, n))
    rng = np.random.default_rng(2)
    syn = rng.integers(0, 2, size=(40, n - 1), dtype=np.uint8)
    rule = LayeredMinSumModel(Hd, prior, 12)
    assert rule.K == 2 and rule.layers == [list(range(0, n - 1, 2)), list(range(1, n - 1, 2))]
    serial = LayeredMinSumModel(Hd, prior, 12, layers=[[i] for i in rule.layers[0] + rule.layers[1]]).decode(syn)
    for g, w in zip(serial, rule.decode(syn)):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert 0 < serial[1].sum()


# ---- ldpc_minsum_create / MinSumDecoder validate before any device work ---------------------------------------------

GOOD = dict(colptr=[0, 2, 3, 5], rowval=[0, 1, 1, 0, 2], s=3, n=3, llr=[1.0, -2.0, 3.0])


def _create(schedule, **kw):
    L = ldpc._capi.lib()
    colptr, rowval = np.asarray(GOOD["colptr"], dtype=np.int64), np.asarray(GOOD["rowval"], dtype=np.int64)
    llr = np.asarray(GOOD["llr"], dtype=np.float32)
    o = ldpc._capi.MinSumOptions()
    o.device = -1
    o.schedule = schedule
    for k, v in kw.items():
        setattr(o, k, v)
    h = ctypes.c_void_p()
    st = L.ldpc_minsum_create(3, 3, 5, colptr.ctypes.data, rowval.ctypes.data, llr.ctypes.data, 10, ctypes.byref(o), ctypes.byref(h))
    msg = L.ldpc_last_error().decode()
    layers = L.ldpc_minsum_layers(h) if st == 0 else None
    if st == 0:
        L.ldpc_minsum_destroy(h)
    else:
        assert not h.value
    return st, msg, layers


def test_schedule_field_of_the_options_struct():
    O = ldpc._capi.MinSumOptions
    assert ctypes.sizeof(O) == 64 and O.schedule.offset == 16 and O.schedule.size == 4 and O.reserved.offset == 20
    assert O().schedule == 0                                              # a zeroed struct: today's behaviour
    for bad in (2, -1, 7, 1 << 20):
        st, msg, _ = _create(bad)
        assert st == INVALID and "schedule" in msg, (bad, st, msg)
    st, msg, _ = _create(2, kernel_variant=1)
    assert st == INVALID
    for schedule, K in ((0, 0), (1, 2)):                                  # checks {0,2}, {0,1}, {2}: 1 and 2 meet 0 only
        st, msg, layers = _create(schedule)
        assert st in (0, NO_DEVICE), (st, msg)
        if st == 0:
            assert layers == K, layers
    assert ldpc._capi.lib().ldpc_minsum_layers(None) == 0


@pytest.mark.parametrize("bad", ["serial", "", "Layered", None, 1, 0, True, b"layered"])
def test_constructor_refuses_another_schedule(bad):
    H = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    with pytest.raises(ValueError):
        ldpc.MinSumDecoder(H, 0.1, 10, schedule=bad)


def test_constructor_takes_both_schedules():
    H = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    for schedule, K in (("flooding", 0), ("layered", 2)):
        try:
            dec = ldpc.MinSumDecoder(H, 0.1, 10, schedule=schedule)
        except ldpc.LdpcError as e:
            assert e.status == NO_DEVICE                                  # validation passed; there is no CPU path
            continue
        assert dec.schedule == schedule and dec.layers == K and dec.info().layers == K and dec.info().schedule == schedule
        dec.close()
