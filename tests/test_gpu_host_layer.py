"""The Python host layer on the GPU, on the smallest inputs at which its marshalling can go wrong: for every decoder the
host entry against the device entry on the same three syndromes, the refusals of the tensor check, and the handle's
lifetime; one sample -> syndromes -> score round of the two trial handles; one gather / commit of the window step.  What
the kernels compute is held against the models elsewhere; here the two entries need only agree in every element."""
import numpy as np
import pytest

import windows_model as wm

pytestmark = pytest.mark.gpu

B = 3
# 6 checks on 13 bits: bit degrees 0 (bit 5) to 4, check degrees 4 and 5
H = np.array([[1, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1],
              [1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1],
              [0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 1],
              [0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1],
              [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0],
              [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0]], dtype=np.uint8)
S, N = H.shape
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)   # Steane: Hx = Hz
ERRORS = np.zeros((B, N), dtype=np.uint8)
ERRORS[1, 3] = ERRORS[2, 0] = ERRORS[2, 7] = ERRORS[2, 5] = 1
SYN = (ERRORS @ H.T % 2).astype(np.uint8)
PAULI_EX = np.array([[0] * 7, [0, 0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 1, 0]], dtype=np.uint8)
PAULI_EZ = np.array([[0, 0, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0] * 7], dtype=np.uint8)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(torch, shape, dtype):
    return torch.full(shape, 7, dtype=dtype, device="cuda")


class Case:
    """One decoder: `make()`, the host call, and the device call as (inputs, output tensors, call)."""

    def __init__(self, make, host, inputs, outputs, device):
        self.make, self.host, self.inputs, self.outputs, self.device = make, host, inputs, outputs, device


def _cases(ldpc, torch):
    u8, i32, f64 = torch.uint8, torch.int32, torch.float64
    plain = lambda: [_out(torch, (B, N), u8), _out(torch, (B,), u8), _out(torch, (B, N), f64), _out(torch, (B,), i32)]  # noqa: E731
    priors = np.random.default_rng(5).uniform(0.5, 4.0, size=(B, N)).astype(np.float32)
    given = np.random.default_rng(6).integers(0, 2, size=(B, N), dtype=np.uint8)

    def minsum():
        dec = ldpc.MinSumDecoder(H, 0.08, 8)
        dec.set_conditional_priors(probs_if0=0.05, probs_if1=0.4)
        return dec

    return {
        "bp": Case(lambda: ldpc.BeliefPropagationDecoder(H, 0.08, 8),
                   lambda d: d.decode_batch_host(SYN, want_llr=True, want_iters=True), [SYN], plain,
                   lambda d, i, o, **kw: d.decode_batch_device(i[0], o[0], o[1], o[2], o[3], **kw)),
        "bpots": Case(lambda: ldpc.BPOTSDecoder(H, 0.08, 8),
                      lambda d: d.decode_batch_host(SYN), [SYN],
                      lambda: [_out(torch, (B, N), u8), _out(torch, (B,), u8), _out(torch, (B,), i32)],
                      lambda d, i, o, **kw: d.decode_batch_device(i[0], o[0], o[1], o[2], **kw)),
        "bitflip": Case(lambda: ldpc.BitFlipDecoder(H, 0.08, 8, seed=3),
                        lambda d: d.decode_batch_host(SYN, column0=40), [SYN],
                        lambda: [_out(torch, (B, N), u8), _out(torch, (B,), u8), _out(torch, (B,), i32), _out(torch, (B,), u8)],
                        lambda d, i, o, **kw: d.decode_batch_device(i[0], o[0], o[1], o[2], o[3], column0=40, **kw)),
        "minsum": Case(minsum, lambda d: d.decode_batch_host(SYN, want_llr=True), [SYN], plain,
                       lambda d, i, o, **kw: d.decode_batch_device(i[0], o[0], o[1], o[2], o[3], **kw)),
        "minsum_priors": Case(minsum, lambda d: d.decode_batch_priors_host(SYN, priors, want_llr=True), [SYN, priors], plain,
                              lambda d, i, o, **kw: d.decode_batch_priors_device(i[0], i[1], o[0], o[1], o[2], o[3], **kw)),
        "minsum_given": Case(minsum, lambda d: d.decode_batch_given_host(SYN, given, want_llr=True), [SYN, given], plain,
                             lambda d, i, o, **kw: d.decode_batch_given_device(i[0], i[1], o[0], o[1], o[2], o[3], **kw)),
        "relay": Case(lambda: ldpc.RelayMinSumDecoder(H, 0.08, 4, legs=3, leg_iters=3, stop_after=2, seed=1),
                      lambda d: d.decode_batch_host(SYN, want_llr=True, want_solutions=True), [SYN],
                      lambda: plain() + [_out(torch, (B,), i32)],
                      lambda d, i, o, **kw: d.decode_batch_device(i[0], o[0], o[1], o[2], o[3], o[4], **kw)),
        "pauli": Case(lambda: ldpc.PauliMinSumDecoder(HAMMING, HAMMING, 0.09, 8),
                      lambda d: d.decode_batch_host(PAULI_EZ @ HAMMING.T % 2, PAULI_EX @ HAMMING.T % 2, want_llr=True),
                      [(PAULI_EZ @ HAMMING.T % 2).astype(np.uint8), (PAULI_EX @ HAMMING.T % 2).astype(np.uint8)],
                      lambda: [_out(torch, (B, 7), u8), _out(torch, (B, 7), u8), _out(torch, (B,), u8), _out(torch, (B, 3, 7), f64),
                               _out(torch, (B,), i32)],
                      lambda d, i, o, **kw: d.decode_batch_device(i[0], i[1], o[0], o[1], o[2], o[3], o[4], **kw)),
    }


NAMES = ("bp", "bpots", "bitflip", "minsum", "minsum_priors", "minsum_given", "relay", "pauli")


def _same_elements(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: output {k} of the device entry differs from the host entry's"


@pytest.mark.parametrize("name", NAMES)
def test_host_entry_device_entry_refusals_and_lifetime(ldpc, gpu, name):
    import torch

    case = _cases(ldpc, torch)[name]
    dec = case.make()
    want = case.host(dec)
    assert any(x.any() for x in want[:3]) and want[0].shape[0] == B             # (something was decoded)
    inputs = [_dev(torch, a) for a in case.inputs]
    outs = case.outputs()
    case.device(dec, inputs, outs)
    torch.cuda.synchronize()
    _same_elements(outs, want, name)
    if name == "bp":
        # a stream given outright is the one the call runs on
        side = torch.cuda.Stream()
        outs = case.outputs()
        side.wait_stream(torch.cuda.current_stream())
        case.device(dec, inputs, outs, stream=side.cuda_stream)
        side.synchronize()
        _same_elements(outs, want, name + " on a side stream")
    # what the tensor check refuses: every argument in turn as a wrong dtype, a non-contiguous view and a CPU tensor
    counted = getattr(dec, "columns_decoded", None)
    for group, tensors in (("input", inputs), ("output", outs)):
        for k, good in enumerate(tensors):
            wrong = (good.to(torch.int16), good.cpu())
            if good.dim() == 2:
                wrong += (torch.zeros((good.shape[1], good.shape[0]), dtype=good.dtype, device="cuda").t(),
                          good[:, :-1].contiguous(), good[:-1])
            else:
                wrong += (torch.zeros(2 * good.numel(), dtype=good.dtype, device="cuda").view(*good.shape[:-1], -1)[..., ::2],)
            for bad in wrong:
                if bad.is_cuda and bad.dtype == good.dtype and bad.shape == good.shape:
                    assert not bad.is_contiguous()
                swapped = [list(inputs), list(outs)]
                swapped[group == "output"][k] = bad
                with pytest.raises(AssertionError):
                    case.device(dec, *swapped)
    assert getattr(dec, "columns_decoded", None) == counted                      # (a refused call decodes no column)
    outs = case.outputs()
    case.device(dec, inputs, outs)                                               # ... and the next correct call succeeds
    torch.cuda.synchronize()
    _same_elements(outs, want, name + " after the refusals")
    # lifetime
    dec.close()
    assert dec._h is None
    dec.close()
    for call in (lambda: case.host(dec), lambda: case.device(dec, inputs, case.outputs())):
        with pytest.raises(ldpc.LdpcError) as ei:
            call()
        assert ei.value.status == 1 and "NULL" in ei.value.message, ei.value


def test_optional_outputs_may_be_left_out(ldpc, gpu):
    import torch

    syn = _dev(torch, SYN)
    for name in ("bp", "bpots", "bitflip", "minsum", "relay"):
        case = _cases(ldpc, torch)[name]
        dec = case.make()
        want = case.host(dec)
        err, conv = _out(torch, (B, N), torch.uint8), _out(torch, (B,), torch.uint8)
        if name == "bitflip":
            dec.decode_batch_device(syn, err, conv, column0=40)
        else:
            dec.decode_batch_device(syn, err, conv)
        torch.cuda.synchronize()
        _same_elements([err, conv], want[:2], name + " without the optional outputs")
        dec.close()


def test_decode_and_batchdecode_keep_what_each_scratch_keeps(ldpc, gpu):
    """The shared decode_ / batchdecode_ pair: min-sum and relay keep err and log_probabs of the last column, bit-flip
    keeps err, BP-OTS keeps nothing and returns an Int copy."""
    import torch

    cases = _cases(ldpc, torch)
    for name in ("minsum", "relay", "bitflip", "bpots"):
        dec = cases[name].make()
        if name == "bitflip":
            dec.columns_decoded = 40
        want = cases[name].host(dec) if name != "bitflip" else dec.decode_batch_host(SYN, column0=40)
        errors, success = np.full((N, B), 9, dtype=np.int32), np.zeros(B, dtype=np.bool_)
        got_e, got_s = dec.batchdecode_(SYN.T, errors, success)
        assert got_e is errors and got_s is success
        assert np.array_equal(errors, want[0].T) and np.array_equal(success, want[1].astype(bool))
        if name == "bpots":
            assert not hasattr(dec, "scratch")
        else:
            assert np.array_equal(dec.scratch.err, want[0][-1])
        if name in ("minsum", "relay"):
            assert np.array_equal(dec.scratch.log_probabs, want[2][-1])
        if name == "bitflip":
            assert dec.columns_decoded == 40 + B
            dec.columns_decoded = 41
        guess, ok = dec.decode_(SYN[1])
        assert np.array_equal(guess, want[0][1]) and ok == bool(want[1][1])
        if name == "bpots":
            assert guess.dtype == np.int64
        else:
            assert guess is dec.scratch.err
        if name in ("minsum", "relay"):
            assert np.array_equal(dec.scratch.log_probabs, want[2][1])
        with pytest.raises(IndexError, match=f"syndrome has length 5, decoder has {S} checks"):
            dec.decode_(SYN[1][:5])
        if name == "bitflip":
            dec.columns_decoded = 40
        _, fresh = dec.batchdecode_(SYN.T, errors)
        assert fresh.dtype == np.bool_ and np.array_equal(fresh, success)
        dec.close()


def test_trials_round(ldpc, gpu):
    import torch

    t = ldpc.Trials(H, logicals=np.ones((1, N), dtype=np.uint8))
    e0, s0, s1 = _out(torch, (B, N), torch.uint8), _out(torch, (B, S), torch.uint8), _out(torch, (B, S), torch.uint8)
    e, s = t.sample(B, 0.3, seed=4, column0=2, out=(e0, s0))
    assert e is e0 and s is s0
    assert t.syndromes(e, out=s1) is s1
    he, hs = t.sample_host(B, 0.3, seed=4, column0=2)
    assert he.any() and np.array_equal(e.cpu().numpy(), he) and np.array_equal(s.cpu().numpy(), hs)
    assert np.array_equal(hs, he @ H.T % 2) and np.array_equal(s1.cpu().numpy(), hs)
    e_only, none = t.sample(B, 0.3, seed=4, column0=2, out=(_out(torch, (B, N), torch.uint8), None))
    assert none is None and np.array_equal(e_only.cpu().numpy(), he)
    flags, counts = _out(torch, (B,), torch.uint8), torch.zeros(4, dtype=torch.int64, device="cuda")
    guess = e.clone()
    guess[1, 0] ^= 1
    f, c = t.score(e, e, flags=flags, counts=counts)
    assert f is flags and c is counts and counts.cpu().tolist() == [B, 0, 0, 0] and flags.cpu().tolist() == [0] * B
    f2, c2 = t.score(guess, e, counts=counts)
    assert c2 is counts and counts.cpu().tolist() == [2 * B, 1, 1, 1] and f2.cpu().tolist()[1] != 0
    hf, hc = t.score_host(guess.cpu().numpy(), he)
    assert np.array_equal(hf, f2.cpu().numpy()) and hc.tolist() == [B, 1, 1, 1]
    assert t.score(guess, e, want_flags=False)[0] is None
    for bad in (e.to(torch.int32), e.cpu(), e[:, :-1], torch.zeros((N, B), dtype=torch.uint8, device="cuda").t()):
        with pytest.raises(AssertionError):
            t.syndromes(bad)
        with pytest.raises(AssertionError):
            t.score(bad, e)
    with pytest.raises(AssertionError):
        t.score(e, e, counts=torch.zeros(4, dtype=torch.int32, device="cuda"))
    t.close()
    t.close()
    with pytest.raises(ldpc.LdpcError) as ei:
        t.sample(B, 0.3)
    assert ei.value.status == 1


def test_css_trials_round(ldpc, gpu):
    import torch

    u8 = torch.uint8
    t = ldpc.CSSTrials(HAMMING, HAMMING)
    out = (_out(torch, (B, 7), u8), _out(torch, (B, 7), u8), _out(torch, (B, 3), u8), _out(torch, (B, 3), u8))
    got = t.sample(B, (0.2, 0.1, 0.15), seed=9, column0=1, out=out)
    assert all(g is o for g, o in zip(got, out))
    ex, ez, sx, sz = got
    hex_, hez, hsx, hsz = t.sample_host(B, (0.2, 0.1, 0.15), seed=9, column0=1)
    assert (hex_.any() or hez.any()) and all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got, (hex_, hez, hsx, hsz)))
    assert np.array_equal(hsx, hez @ HAMMING.T % 2) and np.array_equal(hsz, hex_ @ HAMMING.T % 2)
    again = (_out(torch, (B, 3), u8), _out(torch, (B, 3), u8))
    sx2, sz2 = t.syndromes(ex, ez, out=again)
    assert sx2 is again[0] and sz2 is again[1] and torch.equal(sx2, sx) and torch.equal(sz2, sz)
    flags, counts = _out(torch, (B,), u8), torch.zeros(6, dtype=torch.int64, device="cuda")
    f, c = t.score(ex, ez, ex, ez, flags=flags, counts=counts)
    assert f is flags and c is counts and counts.cpu().tolist() == [B, 0, 0, 0, 0, 0] and flags.cpu().tolist() == [0] * B
    gx = ex.clone()
    gx[2, 6] ^= 1
    f2, c2 = t.score(gx, ez, ex, ez, counts=counts)
    hf, hc = t.score_host(gx.cpu().numpy(), hez, hex_, hez)
    assert c2 is counts and counts.cpu().tolist()[:3] == [2 * B, 1, 1] and np.array_equal(f2.cpu().numpy(), hf) and hc.tolist()[:3] == [B, 1, 1]
    for bad in (ex.to(torch.int32), ex.cpu(), ex[:, :-1], torch.zeros((7, B), dtype=u8, device="cuda").t()):
        with pytest.raises(AssertionError):
            t.syndromes(bad, ez)
        with pytest.raises(AssertionError):
            t.score(gx, bad, ex, ez)
    t.close()
    t.close()
    with pytest.raises(ldpc.LdpcError) as ei:
        t.syndromes(ex, ez)
    assert ei.value.status == 1


def test_window_step_gather_and_commit(ldpc, gpu):
    import scipy.sparse as sp
    import torch

    Hc = sp.csc_matrix(H)
    first = np.array([Hc.indices[Hc.indptr[j]] if Hc.indptr[j + 1] > Hc.indptr[j] else -1 for j in range(N)])
    windows = [dict(det=np.arange(0, 4), mech=np.flatnonzero((first >= 0) & (first < 2)), commit=None),
               dict(det=np.arange(2, 6), mech=np.flatnonzero(first >= 2), commit=None)]
    for w in windows:
        w["commit"] = np.arange(w["mech"].size, dtype=np.int64)
    assert windows[0]["mech"].size and windows[1]["mech"].size and first[5] == -1
    step = ldpc.WindowStep(H, [w["det"] for w in windows], [w["mech"] for w in windows], [w["commit"] for w in windows])
    assert len(step) == 2
    rng = np.random.default_rng(2)
    residual = SYN.copy()
    guess, conv = np.full((B, N), 9, dtype=np.uint8), np.ones(B, dtype=np.uint8)
    d_res, d_guess, d_conv = _dev(torch, residual), _dev(torch, guess), _dev(torch, conv)
    out = _out(torch, (B, 4), torch.uint8)
    assert step.gather(0, d_res, out=out) is out
    assert np.array_equal(out.cpu().numpy(), wm.gather(residual, windows[0]["det"]))
    assert np.array_equal(step.gather(1, d_res).cpu().numpy(), wm.gather(residual, windows[1]["det"]))
    for k in (0, 1):
        win_guess = rng.integers(0, 2, size=(B, windows[k]["mech"].size), dtype=np.uint8)
        win_conv = np.array([1, 0, 1], dtype=np.uint8) if k == 0 else np.array([1, 1, 0], dtype=np.uint8)
        nxt = _out(torch, (B, 4), torch.uint8) if k == 0 else None
        step.commit(k, _dev(torch, win_guess), d_res, d_guess, win_conv=_dev(torch, win_conv), conv=d_conv, next_syndromes=nxt)
        want_next = wm.commit(H, windows, k, win_guess, residual, guess, win_conv, conv, want_next=k == 0)
        assert np.array_equal(d_res.cpu().numpy(), residual) and np.array_equal(d_guess.cpu().numpy(), guess)
        assert np.array_equal(d_conv.cpu().numpy(), conv)
        if k == 0:
            assert np.array_equal(nxt.cpu().numpy(), want_next)
    assert conv.tolist() == [1, 0, 0] and (guess[:, 5] == 9).all()               # (bit 5 is in no window)
    for bad in (d_res.to(torch.int32), d_res.cpu(), d_res[:, :-1], torch.zeros((S, B), dtype=torch.uint8, device="cuda").t()):
        with pytest.raises(AssertionError):
            step.gather(0, bad)
    with pytest.raises(AssertionError):
        step.commit(1, _dev(torch, win_guess), d_res, d_guess, conv=d_conv.to(torch.int32))
    assert np.array_equal(d_res.cpu().numpy(), residual)
    step.close()
    step.close()
    with pytest.raises(ldpc.LdpcError) as ei:
        step.gather(0, d_res)
    assert ei.value.status == 1
