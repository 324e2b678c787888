"""Device form of the OSD step on the GPU (ldpc_osd_postprocess_batch_device; csrc/osd_kernels.hpp) against the CPU
model of its stated key rule (tests/osd_model.py).  Kernel and model are given the SAME bits -- the GPU BP decoder's
own hard decisions and exact LLRs -- so equality is exact: every element of every syndrome, nothing left out."""
import numpy as np
import pytest
import scipy.sparse as sp

from osd_model import osd_model_postprocess

pytestmark = pytest.mark.gpu


def _dense(H):
    return np.asarray(sp.csc_matrix(H).todense()).astype(np.uint8)


def _syn_of(Hd, out):
    return ((out.astype(np.int64) @ Hd.T.astype(np.int64)) % 2).astype(np.uint8)


def _bp(ldpc, H, per, iters, syn):
    dec = ldpc.BeliefPropagationDecoder(H, per, iters, device=0, llr_exact=True)
    err, conv, llr, _ = dec.decode_batch_host(syn, want_llr=True)
    dec.close()
    return err, conv, llr


def _device(ldpc, H, order, syn, err, llr, variant=0, tier=None, inplace=False, post=None):
    import torch

    own = post is None
    if own:
        post = ldpc.OSDPostProcessor(H, order)
        post.prepare_device(0, variant)
    if tier is not None:
        assert post.kernel == tier, (post.kernel, tier)
    d_syn = torch.from_numpy(np.ascontiguousarray(syn, dtype=np.uint8)).to("cuda:0")
    d_err = torch.from_numpy(np.ascontiguousarray(err, dtype=np.uint8)).to("cuda:0")
    d_llr = torch.from_numpy(np.ascontiguousarray(llr, dtype=np.float64)).to("cuda:0")
    out = post.postprocess_device(d_syn, d_err, d_llr, out=d_err if inplace else None)
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(d_err.cpu().numpy(), err), "bp_errors was written by an out-of-place call"
    res = out.cpu().numpy()
    if own:
        post.close()
    return res


def _against_model(ldpc, H, order, syn, err, llr, consistent=True, **kw):
    Hd = _dense(H)
    out = _device(ldpc, H, order, syn, err, llr, **kw)
    for b in range(syn.shape[0]):
        ref = osd_model_postprocess(Hd, syn[b], err[b], llr[b], order)
        assert np.array_equal(out[b], ref), f"order {order} syndrome {b}: the kernel differs from the model"
    if consistent:
        assert np.array_equal(_syn_of(Hd, out), (syn != 0).astype(np.uint8)), "an output does not reproduce its syndrome"
    return out


_BB = {}


def _bb72_case(ldpc, rate):
    if rate not in _BB:
        HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
        H = sp.csc_matrix(HX)
        E = ldpc.codes.random_errors(72, 4000, rate, seed=int(rate * 100))
        syn = ldpc.codes.syndromes_of(H, E)
        _BB[rate] = (H, syn) + _bp(ldpc, H, 0.005, 50, syn)
    return _BB[rate]


@pytest.mark.parametrize("order", [0, 1, 3, 5, 10])
@pytest.mark.parametrize("rate", [0.04, 0.06])
def test_tier1_bb72(ldpc, gpu, rate, order):
    """One wave per syndrome; BB-72 H_X has rank 30 of 36 (dependent rows)."""
    H, syn, err, conv, llr = _bb72_case(ldpc, rate)
    assert 0.01 < 1 - conv.mean() < 0.9
    _against_model(ldpc, H, order, syn, err, llr, tier=1)


@pytest.mark.parametrize("order", [0, 3])
def test_tier3_forced_on_bb72_equals_tier1(ldpc, gpu, order):
    H, syn, err, conv, llr = _bb72_case(ldpc, 0.04)
    a = _device(ldpc, H, order, syn, err, llr, tier=1)
    b = _device(ldpc, H, order, syn, err, llr, variant=3, tier=3)
    c = _device(ldpc, H, order, syn, err, llr, variant=2, tier=2)
    assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("per,B", [(0.03, 64), (0.2, 16)])
def test_tier2_reference_test_code(ldpc, gpu, per, B, order):
    """parity_check_matrix(1000, 10, 9), the reference's own test code: 900 rows x 16 words in dynamic LDS."""
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    E = ldpc.codes.random_errors(1000, B, per, seed=11)
    syn = ldpc.codes.syndromes_of(H, E)
    err, conv, llr = _bp(ldpc, H, per, 50, syn)
    if per == 0.2:
        assert not conv.any()
    _against_model(ldpc, H, order, syn, err, llr, tier=2)


@pytest.mark.parametrize("order", [0, 4])
def test_tier2_many_unconverged(ldpc, gpu, order):
    H = ldpc.codes.parity_check_csc(200, 10, 9)
    E = ldpc.codes.random_errors(200, 512, 0.1, seed=12)
    syn = ldpc.codes.syndromes_of(H, E)
    err, conv, llr = _bp(ldpc, H, 0.1, 50, syn)
    assert 1 - conv.mean() > 0.3
    _against_model(ldpc, H, order, syn, err, llr, tier=2)


@pytest.mark.parametrize("order", [0, 2])
def test_tier3_beyond_the_lds(ldpc, gpu, order):
    """parity_check_csc(4000, 10, 5): 2000 rows x 63 words, about 1 MiB of working rows per syndrome."""
    H = ldpc.codes.parity_check_csc(4000, 10, 5)
    E = ldpc.codes.random_errors(4000, 8, 0.1, seed=13)
    syn = ldpc.codes.syndromes_of(H, E)
    err, conv, llr = _bp(ldpc, H, 0.1, 30, syn)
    _against_model(ldpc, H, order, syn, err, llr, tier=3)


def test_rank_deficient_irregular_and_clamped(ldpc, gpu):
    """The irregular 14 x 30 matrices (an empty row) at orders 0, 1, 3, 7, and osd_order > n - rank (:174-177)."""
    rng = np.random.default_rng(3)
    for trial in range(6):
        Hd = (rng.random((14, 30)) < 0.2).astype(np.uint8)
        Hd[0, :] = 0
        H = sp.csc_matrix(Hd)
        E = (rng.random((12, 30)) < 0.15).astype(np.uint8)
        syn = ldpc.codes.syndromes_of(H, E)
        err, conv, llr = _bp(ldpc, H, 0.1, 10, syn)
        for order in (0, 1, 3, 7):
            for variant in (0, 2, 3):
                _against_model(ldpc, H, order, syn, err, llr, variant=variant)
    Hd = np.eye(5, 7, dtype=np.uint8)
    Hd[:, 5] = 1
    H = sp.csc_matrix(Hd)
    E = np.zeros((3, 7), dtype=np.uint8)
    E[0, 5] = 1
    E[1, 0] = E[1, 6] = 1
    syn = ldpc.codes.syndromes_of(H, E)
    err, conv, llr = _bp(ldpc, H, 0.1, 5, syn)
    for variant in (0, 2, 3):
        _against_model(ldpc, H, 6, syn, err, llr, variant=variant)


@pytest.mark.parametrize("size", [1, 63, 64, 65])
def test_word_boundaries_in_rows_and_columns(ldpc, gpu, size):
    """s or n of 1 / 63 / 64 / 65 (0 is the next test); the inputs are drawn, not decoded: any bp_err / LLR row is a
    valid input (the syndromes are those of random errors, hence consistent)."""
    rng = np.random.default_rng(size)
    for s, n in ((size, 90), (40, size), (size, size)):
        Hd = (rng.random((s, n)) < min(0.5, 4.0 / max(min(s, n), 1) + 0.05)).astype(np.uint8)
        H = sp.csc_matrix(Hd)
        B = 40
        E = (rng.random((B, n)) < 0.1).astype(np.uint8)
        syn = _syn_of(Hd, E)
        err = (rng.random((B, n)) < 0.1).astype(np.uint8)
        llr = -np.exp(rng.uniform(-8, 1, (B, n)))
        llr[rng.random((B, n)) < 0.3] = llr[0, 0]   # ties
        for order in (0, 3):
            for variant in (0, 2, 3):
                _against_model(ldpc, H, order, syn, err, llr, variant=variant)


def test_zero_rows_or_columns_and_batch_0_and_1(ldpc, gpu):
    import torch

    # s = 0: no equation; order 0 returns BP's estimate, order > 0 searches the n free columns
    H = sp.csc_matrix(np.zeros((0, 9), dtype=np.uint8))
    rng = np.random.default_rng(5)
    err = (rng.random((7, 9)) < 0.4).astype(np.uint8)
    llr = -np.exp(rng.uniform(-5, 1, (7, 9)))
    syn = np.zeros((7, 0), dtype=np.uint8)
    for order in (0, 2):
        _against_model(ldpc, H, order, syn, err, llr)
    # n = 0: nothing to write
    post = ldpc.OSDPostProcessor(sp.csc_matrix(np.zeros((4, 0), dtype=np.uint8)), 0)
    post.prepare_device(0)
    z8 = torch.zeros((3, 0), dtype=torch.uint8, device="cuda:0")
    out = post.postprocess_device(torch.zeros((3, 4), dtype=torch.uint8, device="cuda:0"), z8,
                                  torch.zeros((3, 0), dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 0)
    post.close()
    # batch 0 touches nothing, batch 1 works
    H, syn, err, conv, llr = _bb72_case(ldpc, 0.04)
    post = ldpc.OSDPostProcessor(H, 2)
    assert post.kernel == 0 and post.prepare_device(0) == 1
    with pytest.raises(ldpc.LdpcError):
        post.prepare_device(0)          # once per handle
    e0 = torch.zeros((0, 72), dtype=torch.uint8, device="cuda:0")
    post.postprocess_device(torch.zeros((0, 36), dtype=torch.uint8, device="cuda:0"), e0,
                            torch.zeros((0, 72), dtype=torch.float64, device="cuda:0"))
    b = int(np.nonzero(conv == 0)[0][0])
    one = _device(ldpc, H, 2, syn[b:b + 1], err[b:b + 1], llr[b:b + 1], post=post)
    assert np.array_equal(one[0], osd_model_postprocess(_dense(H), syn[b], err[b], llr[b], 2))
    post.close()


@pytest.mark.parametrize("order", [0, 3])
def test_in_place_twice_and_on_two_streams(ldpc, gpu, order):
    import torch

    H, syn, err, conv, llr = _bb72_case(ldpc, 0.06)
    for variant in (0, 3):
        post = ldpc.OSDPostProcessor(H, order)
        post.prepare_device(0, variant)
        a = _device(ldpc, H, order, syn, err, llr, post=post)
        b = _device(ldpc, H, order, syn, err, llr, post=post, inplace=True)
        assert np.array_equal(a, b), "in place differs from out of place"
        # the same handle on two streams, back to back (tier 3: they share the workspace, so they must run in call order)
        d_syn = torch.from_numpy(syn).to("cuda:0")
        d_err = torch.from_numpy(err).to("cuda:0")
        d_llr = torch.from_numpy(llr).to("cuda:0")
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s1):
            o1 = post.postprocess_device(d_syn, d_err, d_llr)
        with torch.cuda.stream(s2):
            o2 = post.postprocess_device(d_syn[:1000].contiguous(), d_err[:1000].contiguous(), d_llr[:1000].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(o1.cpu().numpy(), a) and np.array_equal(o2.cpu().numpy(), a[:1000])
        post.close()


def test_nan_and_infinite_llr_rows_and_non_binary_syndrome(ldpc, gpu):
    """A NaN LLR orders last among all columns by ascending index; +-Inf are the most reliable; a syndrome entry that
    is not 0 counts as 1."""
    H, syn, err, conv, llr = _bb72_case(ldpc, 0.06)
    idx = np.nonzero(conv == 0)[0][:200]
    syn, err, llr = syn[idx].copy(), err[idx].copy(), llr[idx].copy()
    rng = np.random.default_rng(9)
    llr[rng.random(llr.shape) < 0.1] = np.nan
    llr[rng.random(llr.shape) < 0.05] = -np.inf
    llr[rng.random(llr.shape) < 0.05] = np.inf
    llr[0, :] = np.nan
    llr[1, :] = -np.inf
    syn[2:40][syn[2:40] == 1] = 7
    for order in (0, 3):
        for variant in (0, 2, 3):
            _against_model(ldpc, H, order, syn, err, llr, variant=variant)


@pytest.mark.parametrize("order", [0, 2])
def test_end_to_end_device_resident_pipeline(ldpc, gpu, order):
    """BeliefPropagationOSDDecoder(..., osd="device").batchdecode_device on 20,000 BB-72 syndromes: conv and sent as
    the osd="host" decoder's, estimates equal to the model chain, and equal to the host decoder's on all but at most
    0.5 % of the syndromes (where libm's exp orders two columns differently), each of which satisfies H e = s."""
    import torch

    HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    H = sp.csc_matrix(HX)
    Hd = _dense(H)
    B = 20000
    E = ldpc.codes.random_errors(72, B, 0.03, seed=5)
    syn = ldpc.codes.syndromes_of(H, E)
    d_syn = torch.from_numpy(syn).to("cuda:0")
    host = ldpc.BeliefPropagationOSDDecoder(HX, 0.005, 50, osd_order=order)
    dev = ldpc.BeliefPropagationOSDDecoder(HX, 0.005, 50, osd_order=order, osd="device")
    assert dev._osd.kernel == 1 and host._osd.kernel == 0
    herr, hconv, hsent = host.batchdecode_device(d_syn)
    derr, dconv, dsent = dev.batchdecode_device(d_syn)
    torch.cuda.synchronize()
    assert derr.is_cuda and dconv.is_cuda
    herr, hconv, derr, dconv = herr.cpu().numpy(), hconv.cpu().numpy(), derr.cpu().numpy(), dconv.cpu().numpy()
    assert np.array_equal(dconv, hconv) and dsent == hsent == (B if order else int((hconv == 0).sum()))
    bperr, bpconv, bpllr = _bp(ldpc, H, 0.005, 50, syn)
    assert np.array_equal(bpconv, hconv)
    for b in range(B):
        ref = bperr[b] if (order == 0 and bpconv[b]) else osd_model_postprocess(Hd, syn[b], bperr[b], bpllr[b], order)
        assert np.array_equal(derr[b], ref), f"syndrome {b} differs from the model chain"
    assert np.array_equal(_syn_of(Hd, derr), syn)
    differ = int((derr != herr).any(axis=1).sum())
    print(f"order {order}: device and host estimates differ on {differ} of {B} syndromes")
    assert differ <= 0.005 * B
    # the host-array entries with osd="device" go through the same kernel
    out = np.zeros((72, 500), dtype=np.uint8)
    g, c = dev.batchdecode_(syn[:500].T, out)
    assert np.array_equal(g.T, derr[:500]) and np.array_equal(c, dconv[:500].astype(bool))
    g1, c1 = dev.decode_(syn[7])
    assert g1.dtype == np.bool_ and np.array_equal(g1.astype(np.uint8), derr[7]) and c1 == bool(dconv[7])


@pytest.mark.parametrize("order", [0, 2, 3, 4, 5])
def test_reference_exact_recovery_at_low_error_rate(ldpc, gpu, order):
    """test_bposd_decoder.jl:6-34 with the device form: per = 0.01 -> guess == err."""
    rng = np.random.default_rng(order)
    H = ldpc.parity_check_matrix(1000, 10, 9)
    err = rng.random(1000) < 0.01
    syn = (H.astype(np.int64) @ err.astype(np.int64)) % 2
    dec = ldpc.BeliefPropagationOSDDecoder(H, 0.01, 100, osd_order=order, osd="device")
    assert dec._osd.kernel == 2
    guess, success = dec.decode_(syn)
    assert guess.dtype == np.bool_ and np.array_equal(guess, err) and success is True


def test_reference_syndrome_consistency_at_high_error_rate(ldpc, gpu):
    """test_bposd_decoder.jl:37-63: per = 0.2, BP fails, the guess still satisfies the syndrome; batch form."""
    rng = np.random.default_rng(3)
    H = ldpc.parity_check_matrix(1000, 10, 9)
    errors = rng.random((1000, 10)) < 0.2
    syndromes = (H.astype(np.int64) @ errors.astype(np.int64)) % 2
    dec = ldpc.BeliefPropagationOSDDecoder(H, 0.2, 100, osd="device")
    guesses, successes = ldpc.batchdecode_(dec, syndromes, np.zeros_like(errors))
    for i in range(10):
        assert np.array_equal((H.astype(np.int64) @ guesses[:, i].astype(np.int64)) % 2, syndromes[:, i])
    assert successes.dtype == np.bool_ and len(successes) == 10
