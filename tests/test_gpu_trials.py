"""Monte-Carlo trial steps on the GPU.  Every comparison is against the CPU model (tests/trials_model.py: the three rules
of include/ldpc_mi355x.h restated in numpy) and is exact in every element: the path is integer arithmetic with one
legal outcome."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import trials_model as tm

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 257)
COLUMN0S = (0, 5, 1 << 40)
PERS = (0.0, 1.0, 0.5, 0.02, 1e-12)
SEEDS = (0, 0xDEADBEEFCAFE1234)


def _graph_a(ldpc):
    return ldpc.codes.parity_check_csc(1000, 10, 9)     # 900 x 1000: n no multiple of 16 or 64


def _graph_b():
    """37 x 131, seeded: check 3 empty, bit 11 empty, check 20 with 100 entries (more than a wave), odd n."""
    rng = np.random.default_rng(20240611)
    A = (rng.random((37, 131)) < 0.08).astype(np.uint8)
    A[20, :] = 0
    A[20, np.delete(np.arange(131), 11)[rng.choice(130, size=100, replace=False)]] = 1
    A[3, :] = 0
    A[:, 11] = 0
    assert A[20].sum() == 100 and A[3].sum() == 0 and A[:, 11].sum() == 0
    return sp.csc_matrix(A)


def _graph_c(ldpc, nl):
    HX, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    rng = np.random.default_rng(72 + nl)
    return sp.csc_matrix(HX), sp.csc_matrix((rng.random((nl, 72)) < 0.2).astype(np.uint8))


def _np(x):
    return x.cpu().numpy()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} elements differ from the model, first {bad[:6].tolist()}"


def _sample_cases():
    """Every batch, column0, per and seed at least once, and per x column0 in full at batch 65."""
    cases = [(b, COLUMN0S[i % 3], PERS[i % 5], SEEDS[i % 2]) for i, b in enumerate(BATCHES)]
    cases += [(65, c0, per, SEEDS[(i + 1) % 2]) for i, (c0, per) in enumerate(itertools.product(COLUMN0S, PERS))]
    return cases


@pytest.mark.parametrize("graph", ["A", "B"])
def test_sample_equals_the_model_in_both_tiers(ldpc, gpu, graph):
    H = _graph_a(ldpc) if graph == "A" else _graph_b()
    s, n = H.shape
    t1, t2 = ldpc.Trials(H, kernel_variant=1), ldpc.Trials(H, kernel_variant=2)
    auto = ldpc.Trials(H)
    assert (t1.kernel, t2.kernel, auto.kernel) == (1, 2, 1)
    for B, c0, per, seed in _sample_cases():
        want_e = tm.sample(n, B, per, seed, c0)
        want_s = tm.syndromes(H, want_e)
        e1, s1 = t1.sample(B, per, seed=seed, column0=c0)
        e2, s2 = t2.sample(B, per, seed=seed, column0=c0)
        what = f"graph {graph} batch {B} column0 {c0} per {per} seed {seed:#x}"
        _same(_np(e1), want_e, what + " tier 1 errors")
        _same(_np(s1), want_s, what + " tier 1 syndromes")
        _same(_np(e2), _np(e1), what + " tier 2 errors vs tier 1")
        _same(_np(s2), _np(s1), what + " tier 2 syndromes vs tier 1")
    for t in (t1, t2, auto):
        t.close()


def test_sample_on_bb72_many_columns_per_workgroup(ldpc, gpu):
    H, _ = _graph_c(ldpc, 12)
    t = ldpc.Trials(H)
    assert t.kernel == 1
    for B, c0, per, seed in _sample_cases() + [(4099, 3, 0.05, 1)]:    # the last: more column groups than one pass of a small grid
        want_e = tm.sample(72, B, per, seed, c0)
        e, sy = t.sample(B, per, seed=seed, column0=c0)
        _same(_np(e), want_e, f"BB-72 batch {B} errors")
        _same(_np(sy), tm.syndromes(H, want_e), f"BB-72 batch {B} syndromes")
    t.close()


def test_natural_unlimited_tier(ldpc, gpu):
    """s = 64, n = 2^21 (the image of a column does not fit the LDS), eight seeded entries per check, batch 3."""
    s, n = 64, 1 << 21
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(s), 8)
    cols = np.concatenate([rng.choice(n, size=8, replace=False) for _ in range(s)])
    cols[:3] = (0, n - 1, 4097)
    H = sp.csc_matrix((np.ones(rows.size, dtype=np.uint8), (rows, cols)), shape=(s, n))
    t = ldpc.Trials(H)
    assert t.kernel == 2
    with pytest.raises(ldpc.LdpcError) as ei:
        ldpc.Trials(H, kernel_variant=1)
    assert ei.value.status == 5
    want_e = tm.sample(n, 3, 0.5, seed=9, column0=1)
    want_s = tm.syndromes(H, want_e)
    e, sy = t.sample(3, 0.5, seed=9, column0=1)
    _same(_np(e), want_e, "n 2^21 errors")
    _same(_np(sy), want_s, "n 2^21 syndromes")
    _same(_np(t.syndromes(e)), want_s, "n 2^21 syndromes of given errors")
    g = e.clone()
    g[1, int(cols[0])] ^= 1
    g[2, 12345] ^= 1
    flags, counts = t.score(g, e)
    wf, wc = tm.score(H, None, _np(g), want_e)
    _same(_np(flags), wf, "n 2^21 flags")
    _same(_np(counts), wc, "n 2^21 counts")
    t.close()


def test_null_syndromes_leave_the_guard_untouched_and_no_pointer_needs_an_alignment(ldpc, gpu):
    import torch

    H = _graph_a(ldpc)
    s, n = H.shape
    B = 65
    want_e = tm.sample(n, B, 0.1, seed=3, column0=2)
    want_s = tm.syndromes(H, want_e)
    for variant in (1, 2):
        t = ldpc.Trials(H, kernel_variant=variant)
        for off_e, off_s in ((0, 0), (3, 1), (15, 2), (8, 3)):
            buf_e = torch.full((off_e + B * n + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
            buf_s = torch.full((off_s + B * s + 4096,), 0xCD, dtype=torch.uint8, device="cuda")
            e = buf_e[off_e:off_e + B * n].view(B, n)
            sy = buf_s[off_s:off_s + B * s].view(B, s)
            t.sample(B, 0.1, seed=3, column0=2, out=(e, None))                 # errors only
            _same(_np(e), want_e, f"tier {variant} offset {off_e} errors (no syndromes)")
            assert bool((buf_e[:off_e] == 0xAB).all()) and bool((buf_e[off_e + B * n:] == 0xAB).all())
            assert bool((buf_s == 0xCD).all())
            e.fill_(0xAB)
            t.sample(B, 0.1, seed=3, column0=2, out=(e, sy))
            _same(_np(e), want_e, f"tier {variant} offset {off_e} errors")
            _same(_np(sy), want_s, f"tier {variant} offset {off_s} syndromes")
            assert bool((buf_e[:off_e] == 0xAB).all()) and bool((buf_e[off_e + B * n:] == 0xAB).all())
            assert bool((buf_s[:off_s] == 0xCD).all()) and bool((buf_s[off_s + B * s:] == 0xCD).all())
            sy.fill_(0xCD)
            t.syndromes(e, out=sy)
            _same(_np(sy), want_s, f"tier {variant} offset {off_s} syndromes of given errors")
        t.close()


def test_a_call_split_at_an_odd_column_equals_the_single_call(ldpc, gpu):
    import torch

    H = _graph_b()
    s, n = H.shape
    t = ldpc.Trials(H)
    e, sy = t.sample(257, 0.3, seed=8, column0=1 << 40)
    e2 = torch.empty_like(e)
    s2 = torch.empty_like(sy)
    t.sample(101, 0.3, seed=8, column0=1 << 40, out=(e2[:101], s2[:101]))
    t.sample(156, 0.3, seed=8, column0=(1 << 40) + 101, out=(e2[101:], s2[101:]))
    assert torch.equal(e, e2) and torch.equal(sy, s2)
    _same(_np(e), tm.sample(n, 257, 0.3, 8, 1 << 40), "split call")
    t.close()


@pytest.mark.parametrize("graph", ["A", "B"])
def test_syndromes_of_given_errors_equal_codes_syndromes_of(ldpc, gpu, graph):
    import torch

    H = _graph_a(ldpc) if graph == "A" else _graph_b()
    n = H.shape[1]
    e = ldpc.codes.random_errors(n, 257, 0.1, seed=4)
    want = ldpc.codes.syndromes_of(H, e)
    _same(tm.syndromes(H, e), want, "model vs codes.syndromes_of")
    d_e = torch.from_numpy(e).cuda()
    for variant in (1, 2):
        t = ldpc.Trials(H, kernel_variant=variant)
        _same(_np(t.syndromes(d_e)), want, f"graph {graph} tier {variant}")
        # only the low bit of an error byte counts
        _same(_np(t.syndromes(d_e | 0xFE)), want, f"graph {graph} tier {variant}, high bits set")
        t.close()


def _gf2_kernel(H):
    """A basis of the kernel of H over GF(2) (rows), by Gauss-Jordan elimination on the dense matrix."""
    A = np.asarray(sp.csr_matrix(H).todense()).astype(np.uint8) & 1
    s, n = A.shape
    pivots, r = [], 0
    for c in range(n):
        if r == s:
            break
        p = np.nonzero(A[r:, c])[0]
        if p.size == 0:
            continue
        A[[r, r + p[0]]] = A[[r + p[0], r]]
        rows = np.nonzero(A[:, c])[0]
        rows = rows[rows != r]
        A[rows] ^= A[r]
        pivots.append(c)
        r += 1
    free = [c for c in range(n) if c not in set(pivots)]
    basis = np.zeros((len(free), n), dtype=np.uint8)
    for k, f in enumerate(free):
        basis[k, f] = 1
        for i, pc in enumerate(pivots):
            basis[k, pc] = A[i, f]
    return basis


def _guesses_for(H, errors, seed):
    """Guesses derived from the errors: a third unchanged, a third with seeded flips that include bit 0, bit n - 1 and
    the bits at either side of a multiple of 64, a third with d = a sum of kernel vectors of H (found here)."""
    rng = np.random.default_rng(seed)
    B, n = errors.shape
    g = errors.copy()
    K = _gf2_kernel(H)
    A = np.asarray(sp.csr_matrix(H).todense()).astype(np.int64)
    assert K.shape[0] > 0 and not ((A @ K.T.astype(np.int64)) % 2).any()
    edge = [0, n - 1] + [b for m in range(64, n, 64) for b in (m - 1, m)]
    for i in range(B):
        if i % 3 == 1:
            g[i, edge[(i // 3) % len(edge)]] ^= 1
            g[i, rng.choice(n, size=int(rng.integers(0, 4)), replace=False)] ^= 1
        elif i % 3 == 2:
            d = (K[rng.choice(K.shape[0], size=int(rng.integers(1, 4)), replace=False)].sum(axis=0) % 2).astype(np.uint8)
            g[i] ^= d
    return g


@pytest.mark.parametrize("graph", ["A", "B", "C12", "C70"])
def test_score_equals_the_model_and_counts_accumulate(ldpc, gpu, graph):
    import torch

    L = None
    if graph == "A":
        H = _graph_a(ldpc)
    elif graph == "B":
        H = _graph_b()
    else:
        H, L = _graph_c(ldpc, int(graph[1:]))
    n = H.shape[1]
    B = 257
    errors = tm.sample(n, B, 0.05, seed=21)
    guesses = _guesses_for(H, errors, seed=22)
    wf, wc = tm.score(H, L, guesses, errors)
    assert wc[1] > wc[2] > 0 and wc[0] > wc[1], wc          # columns with bit 0 set and bit 1 clear exist, so do clean ones
    if L is not None:
        assert 0 < wc[3] <= wc[1], wc
    d_g, d_e = torch.from_numpy(guesses).cuda(), torch.from_numpy(errors).cuda()
    for variant in (1, 2):
        t = ldpc.Trials(H, logicals=L, kernel_variant=variant)
        flags, counts = t.score(d_g, d_e)
        _same(_np(flags), wf, f"graph {graph} tier {variant} flags")
        _same(_np(counts), wc, f"graph {graph} tier {variant} counts")
        # a second call on the first 65 columns, no flags: the counts are added to, not zeroed
        f2, counts = t.score(d_g[:65].contiguous(), d_e[:65].contiguous(), counts=counts, want_flags=False)
        assert f2 is None
        _same(_np(counts), wc + tm.score(H, L, guesses[:65], errors[:65])[1], f"graph {graph} tier {variant} accumulated counts")
        # only the low bits count, and guesses at another alignment than the errors take the byte path
        buf = torch.zeros(B * n + 16, dtype=torch.uint8, device="cuda")
        g_off = buf[5:5 + B * n].view(B, n)
        g_off.copy_(d_g | 0xFE)
        flags, _ = t.score(g_off, d_e)
        _same(_np(flags), wf, f"graph {graph} tier {variant} flags, guesses unaligned with high bits")
        t.close()
    if L is not None:
        t = ldpc.Trials(H)                                   # nl = 0: bit 2 never set
        flags, counts = t.score(d_g, d_e)
        _same(_np(flags), wf & 3, f"graph {graph} without logicals")
        assert int(counts[3]) == 0
        t.close()


def test_host_forms_equal_the_device_forms(ldpc, gpu):
    H = _graph_a(ldpc)
    t = ldpc.Trials(H)
    e, sy = t.sample(65, 0.05, seed=2, column0=9)
    he, hs = t.sample_host(65, 0.05, seed=2, column0=9)
    _same(he, _np(e), "sample_host errors")
    _same(hs, _np(sy), "sample_host syndromes")
    g = _guesses_for(H, he, seed=6)
    import torch

    flags, counts = t.score(torch.from_numpy(g).cuda(), e)
    hf, hc = t.score_host(g, he)
    _same(hf, _np(flags), "score_host flags")
    _same(hc, _np(counts), "score_host counts")
    _, hc = t.score_host(g, he, counts=hc)
    _same(hc, 2 * _np(counts), "score_host accumulates")
    _same(hf, tm.score(H, None, g, he)[0], "score_host vs model")
    t.close()


def test_steps_enqueued_on_one_stream_without_host_synchronisation(ldpc, gpu):
    import torch

    H = _graph_a(ldpc)
    B = 300
    t = ldpc.Trials(H)
    dec = ldpc.BeliefPropagationDecoder(H, 0.02, 30)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        e = torch.empty((B, 1000), dtype=torch.uint8, device="cuda")
        sy = torch.empty((B, 900), dtype=torch.uint8, device="cuda")
        g = torch.empty((B, 1000), dtype=torch.uint8, device="cuda")
        conv = torch.empty(B, dtype=torch.uint8, device="cuda")
        t.sample(B, 0.02, seed=4, out=(e, sy))
        dec.decode_batch_device(sy, g, conv)
        flags, counts = t.score(g, e)
    st.synchronize()
    he, hs = t.sample_host(B, 0.02, seed=4)
    hg, hconv, _, _ = dec.decode_batch_host(hs)
    hf, hc = t.score_host(hg, he)
    _same(_np(e), he, "errors"); _same(_np(sy), hs, "syndromes"); _same(_np(g), hg, "guesses")
    _same(_np(conv), hconv, "converged"); _same(_np(flags), hf, "flags"); _same(_np(counts), hc, "counts")
    _same(hf, tm.score(H, None, hg, tm.sample(1000, B, 0.02, 4))[0], "flags vs model")
    t.close(); dec.close()


TRIALS, BATCH, PER = 2000, 512, 0.01


def _host_entry(ldpc, kind, H):
    """(decoder, host batch entry: (syndromes [b][s], first trial) -> (guesses [b][n], converged [b]))."""
    if kind == "bp":
        dec = ldpc.BeliefPropagationDecoder(H, PER, 50)
        return dec, lambda syn, c0: dec.decode_batch_host(syn)[:2]
    if kind == "bposd":
        dec = ldpc.BeliefPropagationOSDDecoder(H, PER, 50, osd_order=2, osd="device")

        def entry(syn, c0):
            out = np.zeros((H.shape[1], syn.shape[0]), dtype=np.uint8)
            _, ok = dec.batchdecode_(syn.T, out)
            return np.ascontiguousarray(out.T), ok.astype(np.uint8)
        return dec, entry
    if kind == "bpots":
        dec = ldpc.BPOTSDecoder(H, PER, 50)
        return dec, lambda syn, c0: dec.decode_batch_host(syn)[:2]
    dec = ldpc.BitFlipDecoder(H, PER, 100, seed=3)
    return dec, lambda syn, c0: dec.decode_batch_host(syn, column0=c0)[:2]


@pytest.mark.parametrize("kind", ["bp", "bposd", "bpots", "bitflip"])
def test_run_trials_equals_model_sampler_host_entry_model_score(ldpc, gpu, kind):
    H = _graph_a(ldpc)
    rng = np.random.default_rng(1)
    L = sp.csc_matrix((rng.random((5, 1000)) < 0.01).astype(np.uint8))
    dec, entry = _host_entry(ldpc, kind, H)
    res = ldpc.run_trials(dec, TRIALS, batch=BATCH, seed=17, logicals=L)     # per: the decoder's
    errors = tm.sample(1000, TRIALS, PER, seed=17)
    syn = tm.syndromes(H, errors)
    want = np.zeros(4, dtype=np.int64)
    not_conv = 0
    for c0 in range(0, TRIALS, BATCH):                                        # the same batches, the last one ragged
        g, conv = entry(syn[c0:c0 + BATCH], c0)
        want += tm.score(H, L, g, errors[c0:c0 + BATCH])[1]
        not_conv += int((np.asarray(conv) == 0).sum())
    print(f"{kind}: {res}")
    assert res == ldpc.TrialResult(TRIALS, int(want[1]), int(want[2]), int(want[3]), not_conv)
    assert res.trials == TRIALS and res.block_error_rate == want[1] / TRIALS
    if kind == "bp":
        assert res.block_errors / res.trials < 0.005                          # the reference's own bound (test_bp_decoder.jl:49)
    dec.close() if hasattr(dec, "close") else None
