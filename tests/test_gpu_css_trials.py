"""CSS-code Monte-Carlo trial steps on the GPU.  Every comparison is against the CPU model (tests/css_trials_model.py: the
three rules of include/ldpc_mi355x.h restated in numpy) and is exact in every element: the path is integer arithmetic
with one legal outcome.

Codes: BB-72 (one wave per column, 5 or 6 pieces, mostly edge pieces), the hypergraph product of
parity_check_matrix(60, 6, 3) (n = 4500: a workgroup per column, whole aligned pieces; batch <= 64 keeps the model cheap)
and a toy pair with n = 17 (less than one piece where the column sits well, odd n, 5 rows each).

A note on the structured guesses of the score test.  Under the stated rule dz is seen by Hx and by Lx, so the harmless
Z-side difference is a row of Hz (a Z stabilizer: Hx Hz' = 0 and Lx is in ker Hz), and the harmless X-side difference is
a row of Hx.  The test asserts "bit 0 only" for those, "bits 0 and 3 only" for a row of Lz in gz and "bits 0 and 2 only"
for a row of Lx in gx; a row of Hx in gz (which Hx need not commute with) is compared with the model like everything else."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm

pytestmark = pytest.mark.gpu

BIG0 = (1 << 40) + 3
RATES = (0.06, (0.001, 0.0, 0.05), (0.0, 0.0, 0.0), (0.0, 0.04, 0.0))   # depolarizing, biased, nothing, Y only
CODES = ("bb72", "hgp", "toy")


@functools.lru_cache(maxsize=None)
def _code(name):
    """(Hx, Hz, Lx, Lz) as csc / dense uint8; computed once per session and never changed."""
    import ldpcdecoders_jl_amd as ldpc

    if name == "bb72":
        Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    elif name == "hgp":
        Hx, Hz = ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(60, 6, 3))
    else:
        # n = 3 * 5 + 1 * 2 = 17; the product has 5 rows of Hx and 6 of Hz, of which the last is dropped (a subset of
        # commuting rows commutes)
        Hx, Hz = ldpc.codes.hypergraph_product(np.array([[1, 1, 1]]), np.array([[1, 1, 0, 1, 0], [0, 1, 1, 0, 1]]))
        Hz = Hz[:5]
    Hx, Hz = sp.csc_matrix(Hx).astype(np.uint8), sp.csc_matrix(Hz).astype(np.uint8)
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    assert Lx.shape[0] == Lz.shape[0] > 0
    return Hx, Hz, Lx, Lz


def _batches(name):
    return (1, 5, 1027) if name == "bb72" else (1, 5)


def _handle(ldpc, name, variant, logicals=True):
    Hx, Hz, Lx, Lz = _code(name)
    return ldpc.CSSTrials(Hx, Hz, logicals=(Lx, Lz) if logicals else False, kernel_variant=variant)


def _np(x):
    return x.cpu().numpy()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} elements differ from the model, first {bad[:6].tolist()}"


def _offset_view(torch, shape, off, fill=0xAB, src=None):
    """A [B][cols] view `off` bytes into a larger allocation filled with `fill` -> (buffer, view)."""
    numel = int(shape[0]) * int(shape[1])
    buf = torch.full((off + numel + 64,), fill, dtype=torch.uint8, device="cuda")
    view = buf[off:off + numel].view(*shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _guard_ok(buf, off, numel, fill=0xAB):
    return bool((buf[:off] == fill).all()) and bool((buf[off + numel:] == fill).all())


# ---- sample and syndromes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CODES)
def test_sample_and_syndromes_equal_the_model_in_both_tiers(ldpc, gpu, name):
    Hx, Hz, _, _ = _code(name)
    n = Hx.shape[1]
    handles = [_handle(ldpc, name, 1), _handle(ldpc, name, 2)]
    assert [t.kernel for t in handles] == [1, 2]
    auto = ldpc.CSSTrials(Hx, Hz, logicals=False)
    assert auto.kernel == 1
    auto.close()
    for k, (B, c0, p) in enumerate((B, c0, p) for B in _batches(name) for c0 in (0, BIG0) for p in RATES):
        seed = (0, 0xDEADBEEFCAFE1234)[k % 2]
        want_ex, want_ez = cm.sample(n, B, p, seed, c0)
        want_sx, want_sz = cm.syndromes(Hx, Hz, want_ex, want_ez)
        if p == RATES[2]:
            assert not want_ex.any() and not want_ez.any()
        if p == RATES[3]:
            assert np.array_equal(want_ex, want_ez)
        for t in handles:
            what = f"{name} tier {t.kernel} batch {B} column0 {c0} p {p} seed {seed:#x}"
            ex, ez, sx, sz = t.sample(B, p, seed=seed, column0=c0)
            _same(_np(ex), want_ex, what + " ex")
            _same(_np(ez), want_ez, what + " ez")
            _same(_np(sx), want_sx, what + " sx")
            _same(_np(sz), want_sz, what + " sz")
            # the syndromes of given errors; only the low bit of an error byte counts
            sx2, sz2 = t.syndromes(ex | 0xFE, ez | 0xFE)
            _same(_np(sx2), want_sx, what + " sx of given errors")
            _same(_np(sz2), want_sz, what + " sz of given errors")
    for t in handles:
        t.close()


def test_x_only_noise_equals_the_one_matrix_sampler(ldpc, gpu):
    """py = pz = 0: ex is Trials.sample's errors at per = px and the same seed, ez is zero."""
    Hx, Hz, _, _ = _code("bb72")
    t, one = _handle(ldpc, "bb72", 0), ldpc.Trials(Hz)
    for px, seed, c0 in ((0.02, 5, 0), (0.5, 0xDEADBEEFCAFE1234, BIG0)):
        ex, ez, _, sz = t.sample(1027, (px, 0.0, 0.0), seed=seed, column0=c0)
        e, s = one.sample(1027, px, seed=seed, column0=c0)
        _same(_np(ex), _np(e), f"px {px} ex vs Trials.sample")
        _same(_np(sz), _np(s), f"px {px} sz vs Trials.sample")
        assert not bool(ez.any())
    t.close(); one.close()


CROSS = [("bb72", 1027), ("hgp", 5)]   # the one-matrix cross-checks: one wave per column, a workgroup per column


@pytest.mark.parametrize("name,B", CROSS)
def test_z_only_noise_equals_the_one_matrix_sampler_on_hx(ldpc, gpu, name, B):
    """px = py = 0: ez is Trials(Hx).sample's errors at per = pz and the same seed, sx its syndromes, ex is zero."""
    Hx = _code(name)[0]
    for variant in (1, 2):
        t, one = _handle(ldpc, name, variant), ldpc.Trials(Hx, kernel_variant=variant)
        assert t.kernel == one.kernel == variant
        for pz, seed, c0 in ((0.02, 5, 0), (0.5, 0xDEADBEEFCAFE1234, BIG0)):
            ex, ez, sx, _ = t.sample(B, (0.0, 0.0, pz), seed=seed, column0=c0)
            e, s = one.sample(B, pz, seed=seed, column0=c0)
            assert bool(e.any())
            _same(_np(ez), _np(e), f"{name} tier {variant} pz {pz} ez vs Trials.sample")
            _same(_np(sx), _np(s), f"{name} tier {variant} pz {pz} sx vs Trials.sample")
            assert not bool(ex.any())
        t.close(); one.close()


def test_a_call_split_at_an_odd_column_equals_the_single_call(ldpc, gpu):
    import torch

    t = _handle(ldpc, "bb72", 0)
    whole = t.sample(257, 0.3, seed=8, column0=BIG0)
    parts = [torch.empty_like(x) for x in whole]
    t.sample(101, 0.3, seed=8, column0=BIG0, out=tuple(x[:101] for x in parts))
    t.sample(156, 0.3, seed=8, column0=BIG0 + 101, out=tuple(x[101:] for x in parts))
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))
    t.close()


def test_null_syndromes_write_errors_only(ldpc, gpu):
    import torch

    for name in ("bb72", "hgp"):
        Hx, Hz, _, _ = _code(name)
        n, B = Hx.shape[1], 5
        want_ex, want_ez = cm.sample(n, B, 0.06, 3, 2)
        want_sx, want_sz = cm.syndromes(Hx, Hz, want_ex, want_ez)
        for variant in (1, 2):
            t = _handle(ldpc, name, variant)
            ex, ez = (torch.empty((B, n), dtype=torch.uint8, device="cuda") for _ in range(2))
            sx = torch.full((B, Hx.shape[0]), 0xCD, dtype=torch.uint8, device="cuda")
            sz = torch.full((B, Hz.shape[0]), 0xCD, dtype=torch.uint8, device="cuda")
            t.sample(B, 0.06, seed=3, column0=2, out=(ex, ez, None, None))
            _same(_np(ex), want_ex, f"{name} tier {variant} ex (no syndromes)")
            _same(_np(ez), want_ez, f"{name} tier {variant} ez (no syndromes)")
            assert bool((sx == 0xCD).all()) and bool((sz == 0xCD).all())
            ex.fill_(0xCD)
            with pytest.raises(ldpc.LdpcError) as ei:                          # one of the two alone: refused, nothing written
                t.sample(B, 0.06, seed=3, column0=2, out=(ex, ez, sx, None))
            assert ei.value.status == 1
            assert bool((ex == 0xCD).all()) and bool((sx == 0xCD).all()) and bool((sz == 0xCD).all())
            t.sample(B, 0.06, seed=3, column0=2, out=(ex, ez, sx, sz))
            _same(_np(sx), want_sx, f"{name} tier {variant} sx")
            _same(_np(sz), want_sz, f"{name} tier {variant} sz")
            t.close()


# ---- alignment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bb72", "hgp"])
def test_no_pointer_needs_an_alignment(ldpc, gpu, name):
    """Views one byte (or more) into a larger allocation: each array offset singly, and all together with different
    offsets; the bytes around every output keep their fill."""
    import torch

    Hx, Hz, Lx, Lz = _code(name)
    n, B = Hx.shape[1], 37 if name == "bb72" else 5
    rx, rz = Hx.shape[0], Hz.shape[0]
    want_ex, want_ez = cm.sample(n, B, 0.06, 4, 1)
    want_sx, want_sz = cm.syndromes(Hx, Hz, want_ex, want_ez)
    rng = np.random.default_rng(7)
    gx, gz = want_ex.copy(), want_ez.copy()
    for i in range(B):                                    # a third unchanged, the others with seeded flips on either side
        if i % 3:
            gx[i, rng.choice(n, size=int(rng.integers(0, 3)), replace=False)] ^= 1
            gz[i, rng.choice(n, size=int(rng.integers(0, 3)), replace=False)] ^= 1
    gx[1, 0] ^= 1; gz[1 % B, n - 1] ^= 1
    want_f, want_c = cm.score(Hx, Hz, Lx, Lz, gx, gz, want_ex, want_ez)
    assert 0 < want_c[1] < B or B == 1
    host = dict(gx=gx | 0xFE, gz=gz | 0xFE, ex=want_ex, ez=want_ez)             # high bits of the guesses set
    for variant in (1, 2):
        t = _handle(ldpc, name, variant)
        for off_ex, off_ez, off_sx, off_sz in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 1, 0, 0), (3, 7, 1, 2), (15, 8, 3, 5)):
            b_ex, ex = _offset_view(torch, (B, n), off_ex)
            b_ez, ez = _offset_view(torch, (B, n), off_ez)
            b_sx, sx = _offset_view(torch, (B, rx), off_sx)
            b_sz, sz = _offset_view(torch, (B, rz), off_sz)
            what = f"{name} tier {variant} offsets ex {off_ex} ez {off_ez} sx {off_sx} sz {off_sz}"
            t.sample(B, 0.06, seed=4, column0=1, out=(ex, ez, sx, sz))
            for got, want, w in ((ex, want_ex, "ex"), (ez, want_ez, "ez"), (sx, want_sx, "sx"), (sz, want_sz, "sz")):
                _same(_np(got), want, f"{what} {w}")
            assert _guard_ok(b_ex, off_ex, B * n) and _guard_ok(b_ez, off_ez, B * n)
            assert _guard_ok(b_sx, off_sx, B * rx) and _guard_ok(b_sz, off_sz, B * rz)
            sx.fill_(0xAB); sz.fill_(0xAB)
            t.syndromes(ex, ez, out=(sx, sz))
            _same(_np(sx), want_sx, what + " sx of given errors")
            _same(_np(sz), want_sz, what + " sz of given errors")
            assert _guard_ok(b_sx, off_sx, B * rx) and _guard_ok(b_sz, off_sz, B * rz)
        singles = [tuple(1 if k == j else 0 for k in range(4)) for j in range(4)]
        for offs in [(0, 0, 0, 0)] + singles + [(1, 2, 3, 5), (15, 9, 4, 1)]:
            dev = {key: _offset_view(torch, (B, n), off, src=torch.from_numpy(host[key]).cuda())[1]
                   for key, off in zip(("gx", "gz", "ex", "ez"), offs)}
            flags, counts = t.score(dev["gx"], dev["gz"], dev["ex"], dev["ez"])
            _same(_np(flags), want_f, f"{name} tier {variant} score offsets {offs} flags")
            _same(_np(counts), want_c, f"{name} tier {variant} score offsets {offs} counts")
        t.close()


# ---- score ----------------------------------------------------------------------------------------------------------
def _structured_guesses(name, ex, ez, seed):
    """Guesses by column i % 8: 0 equal; 1 gz ^ a row of Hz; 2 gz ^ a row of Lz; 3 gx ^ a row of Hx; 4 gx ^ a row of Lx;
    5 one seeded flip in gx; 6 one seeded flip in gz; 7 gz ^ a row of Hx.  -> (gx, gz)."""
    Hx, Hz, Lx, Lz = _code(name)
    rng = np.random.default_rng(seed)
    dHx, dHz = np.asarray(Hx.todense()).astype(np.uint8), np.asarray(Hz.todense()).astype(np.uint8)
    gx, gz = ex.copy(), ez.copy()
    pick = lambda M: M[int(rng.integers(0, M.shape[0]))]   # noqa: E731
    for i in range(ex.shape[0]):
        kind = i % 8
        if kind == 1:
            gz[i] ^= pick(dHz)
        elif kind == 2:
            gz[i] ^= pick(Lz)
        elif kind == 3:
            gx[i] ^= pick(dHx)
        elif kind == 4:
            gx[i] ^= pick(Lx)
        elif kind == 5:
            gx[i, int(rng.integers(0, ex.shape[1]))] ^= 1
        elif kind == 6:
            gz[i, int(rng.integers(0, ex.shape[1]))] ^= 1
        elif kind == 7:
            gz[i] ^= pick(dHx)
    return gx, gz


@pytest.mark.parametrize("name", CODES)
def test_score_equals_the_model_and_counts_accumulate(ldpc, gpu, name):
    import torch

    Hx, Hz, Lx, Lz = _code(name)
    n = Hx.shape[1]
    B = 259 if name == "bb72" else 61
    ex, ez = cm.sample(n, B, 0.06, seed=21)
    gx, gz = _structured_guesses(name, ex, ez, seed=22)
    wf, wc = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    kinds = np.arange(B) % 8
    assert (wf[kinds == 0] == 0).all()                       # guesses = errors
    assert (wf[(kinds == 1) | (kinds == 3)] == 1).all()      # off by a stabilizer: bit 0 only
    assert (wf[kinds == 2] == (1 | 8)).all()                 # off by a row of Lz in gz: a logical Z failure
    assert (wf[kinds == 4] == (1 | 4)).all()                 # off by a row of Lx in gx: a logical X failure
    flips = wf[(kinds == 5) | (kinds == 6)]
    assert (flips & 1).all() and (flips & 2).any()           # a single flip breaks a check (where its qubit has one on that side)
    if name != "toy":
        assert (flips & 2).all()
    assert wc[0] == B and wc[3] <= wc[4] + wc[5] and wc[4] > 0 and wc[5] > 0
    d = [torch.from_numpy(a).cuda() for a in (gx, gz, ex, ez)]
    for variant in (1, 2):
        t = _handle(ldpc, name, variant)
        flags, counts = t.score(*d)
        _same(_np(flags), wf, f"{name} tier {variant} flags")
        _same(_np(counts), wc, f"{name} tier {variant} counts")
        # a second call on the first 33 columns, no flags: the counts are added to, not zeroed
        f2, counts = t.score(*(a[:33].contiguous() for a in d), counts=counts, want_flags=False)
        assert f2 is None
        _same(_np(counts), wc + cm.score(Hx, Hz, Lx, Lz, gx[:33], gz[:33], ex[:33], ez[:33])[1], f"{name} tier {variant} accumulated counts")
        # guesses = errors: nothing set
        flags, counts = t.score(d[2], d[3], d[2], d[3])
        assert not bool(flags.any()) and _np(counts).tolist() == [B, 0, 0, 0, 0, 0]
        t.close()
        t = _handle(ldpc, name, variant, logicals=False)     # nlx = nlz = 0: bits 2 and 3 never set
        flags, counts = t.score(*d)
        _same(_np(flags), wf & 3, f"{name} tier {variant} without logicals")
        _same(_np(counts), [wc[0], wc[1], wc[2], 0, 0, 0], f"{name} tier {variant} counts without logicals")
        t.close()


@pytest.mark.parametrize("name", CODES)
def test_score_at_the_batches_of_the_sample_test(ldpc, gpu, name):
    """Batches 1, 5 and (BB-72) 1027: at 1 a single live column shares its workgroup with three dead slots.  The guesses are
    the structured ones from their sixth column on, so that column 0 of the batch is a single flip, not a clean column."""
    import torch

    Hx, Hz, Lx, Lz = _code(name)
    n = Hx.shape[1]
    handles = [_handle(ldpc, name, 1), _handle(ldpc, name, 2)]
    for B, c0 in zip(_batches(name), (BIG0, 0, BIG0)):
        ex, ez = cm.sample(n, B + 5, 0.06, seed=23, column0=c0)
        gx, gz = _structured_guesses(name, ex, ez, seed=24)
        gx, gz, ex, ez = (np.ascontiguousarray(a[5:]) for a in (gx, gz, ex, ez))
        wf, wc = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
        assert wc[0] == B and wf[0] & 1
        d = [torch.from_numpy(a).cuda() for a in (gx, gz, ex, ez)]
        for t in handles:
            flags, counts = t.score(*d)
            _same(_np(flags), wf, f"{name} tier {t.kernel} batch {B} flags")
            _same(_np(counts), wc, f"{name} tier {t.kernel} batch {B} counts")
    for t in handles:
        t.close()


@pytest.mark.parametrize("name,B", CROSS)
def test_score_with_one_side_clean_equals_the_one_matrix_score(ldpc, gpu, name, B):
    """gz = ez: the joint score is Trials(Hz, Lz).score(gx, ex) (bits 0-2, counts 0, 1, 2, 4; bit 3 never set).  The mirror,
    gx = ex: bits 0 and 1 are those of Trials(Hx, Lx).score(gz, ez), bit 3 is its bit 2 and bit 2 is never set.  On BB-72
    the first runs once more with gx one byte off a 16-byte boundary and ex on one."""
    import torch

    Hx, Hz, Lx, Lz = _code(name)
    n = Hx.shape[1]
    ex, ez = cm.sample(n, B, 0.06, seed=31, column0=BIG0)
    rng = np.random.default_rng(32)

    def guesses(e, stabilizers, logicals):
        """Column i % 5: 0 equal; 1 one flip; 2 ^ a logical row; 3 ^ a stabilizer; 4 a flip and a logical row."""
        g = e.copy()
        for i in range(B):
            if i % 5 in (1, 4):
                g[i, int(rng.integers(0, n))] ^= 1
            if i % 5 in (2, 4):
                g[i] ^= logicals[int(rng.integers(0, logicals.shape[0]))]
            if i % 5 == 3:
                g[i] ^= np.asarray(stabilizers[int(rng.integers(0, stabilizers.shape[0]))].todense()).astype(np.uint8)[0]
        return g

    gx, gz = guesses(ex, sp.csr_matrix(Hx), Lx), guesses(ez, sp.csr_matrix(Hz), Lz)
    d_ex, d_ez, d_gx, d_gz = (torch.from_numpy(a).cuda() for a in (ex, ez, gx, gz))
    gx_off = _offset_view(torch, (B, n), 1, src=d_gx)[1]
    assert d_ex.data_ptr() % 16 == 0 and gx_off.data_ptr() % 16 == 1
    for variant in (1, 2):
        t = _handle(ldpc, name, variant)
        one_z, one_x = ldpc.Trials(Hz, logicals=Lz, kernel_variant=variant), ldpc.Trials(Hx, logicals=Lx, kernel_variant=variant)
        assert t.kernel == one_z.kernel == one_x.kernel == variant
        what = f"{name} tier {variant}"
        wf, wc = one_z.score(d_gx, d_ex)
        wf, wc = _np(wf), _np(wc)
        assert wc[0] == B and all(wc[1:] > 0)                       # every bit of the one-matrix score occurs
        for g in (d_gx, gx_off) if name == "bb72" else (d_gx,):
            flags, counts = t.score(g, d_ez, d_ex, d_ez)
            _same(_np(flags), wf, f"{what} gz = ez, gx at {g.data_ptr() % 16} mod 16: flags vs Trials(Hz, Lz).score")
            _same(_np(counts)[[0, 1, 2, 4]], wc, f"{what} gz = ez: counts 0, 1, 2, 4 vs the one-matrix four")
            assert _np(counts)[5] == 0
        wf, wc = one_x.score(d_gz, d_ez)
        wf, wc = _np(wf), _np(wc)
        assert wc[0] == B and all(wc[1:] > 0)
        flags, counts = t.score(d_ex, d_gz, d_ex, d_ez)
        flags = _np(flags)
        _same(flags & 3, wf & 3, f"{what} gx = ex: bits 0 and 1 vs Trials(Hx, Lx).score")
        _same((flags >> 3) & 1, (wf >> 2) & 1, f"{what} gx = ex: bit 3 vs the one-matrix bit 2")
        assert not (flags & 4).any()
        _same(_np(counts)[[0, 1, 2, 5]], wc, f"{what} gx = ex: counts 0, 1, 2, 5 vs the one-matrix four")
        for h in (t, one_z, one_x):
            h.close()


def test_host_forms_equal_the_device_forms(ldpc, gpu):
    import torch

    Hx, Hz, Lx, Lz = _code("bb72")
    t = _handle(ldpc, "bb72", 0)
    dev = t.sample(65, (0.01, 0.02, 0.03), seed=2, column0=9)
    host = t.sample_host(65, (0.01, 0.02, 0.03), seed=2, column0=9)
    for a, b, w in zip(host, dev, ("ex", "ez", "sx", "sz")):
        _same(a, _np(b), "sample_host " + w)
    gx, gz = _structured_guesses("bb72", host[0], host[1], seed=6)
    flags, counts = t.score(torch.from_numpy(gx).cuda(), torch.from_numpy(gz).cuda(), dev[0], dev[1])
    hf, hc = t.score_host(gx, gz, host[0], host[1])
    _same(hf, _np(flags), "score_host flags")
    _same(hc, _np(counts), "score_host counts")
    _, hc = t.score_host(gx, gz, host[0], host[1], counts=hc)
    _same(hc, 2 * _np(counts), "score_host accumulates")
    _same(hf, cm.score(Hx, Hz, Lx, Lz, gx, gz, host[0], host[1])[0], "score_host vs model")
    t.close()


# ---- order and the whole loop ---------------------------------------------------------------------------------------
def test_calls_on_one_handle_run_in_call_order_across_streams(ldpc, gpu):
    """sample on stream A, then score on stream B with no synchronisation by the user in between: the score sees the
    sampled errors."""
    import torch

    Hx, Hz, Lx, Lz = _code("bb72")
    n, B = 72, 20000
    t = _handle(ldpc, "bb72", 0)
    ex, ez, gx, gz = (torch.zeros((B, n), dtype=torch.uint8, device="cuda") for _ in range(4))
    sx = torch.zeros((B, Hx.shape[0]), dtype=torch.uint8, device="cuda")
    sz = torch.zeros((B, Hz.shape[0]), dtype=torch.uint8, device="cuda")
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    t.sample(B, 0.06, seed=12, out=(ex, ez, sx, sz), stream=sa.cuda_stream)
    t.score(gx, gz, ex, ez, flags=flags, counts=counts, stream=sb.cuda_stream)
    sb.synchronize(); sa.synchronize()
    want_ex, want_ez = cm.sample(n, B, 0.06, 12)
    wf, wc = cm.score(Hx, Hz, Lx, Lz, np.zeros_like(want_ex), np.zeros_like(want_ez), want_ex, want_ez)
    assert wc[1] > B // 2
    _same(_np(ex), want_ex, "ex"); _same(_np(flags), wf, "flags"); _same(_np(counts), wc, "counts")
    t.close()


TRIALS, P = 3000, 0.03


@pytest.mark.parametrize("kind", ["bp", "bitflip"])
def test_run_css_trials_equals_model_sampler_device_decoders_model_score(ldpc, gpu, kind):
    import torch

    Hx, Hz, Lx, Lz = _code("bb72")
    per = 2 * P / 3                                     # either side's marginal under depolarizing noise
    if kind == "bp":
        make = lambda H: ldpc.BeliefPropagationDecoder(H, per, 30)   # noqa: E731
    else:
        make = lambda H: ldpc.BitFlipDecoder(H, per, 50, tie_break="random", seed=3)   # noqa: E731
    dec_hx, dec_hz = make(Hx), make(Hz)
    res_a = ldpc.run_css_trials(dec_hx, dec_hz, TRIALS, P, batch=1024, seed=17)
    res_b = ldpc.run_css_trials(dec_hx, dec_hz, TRIALS, P, batch=777, seed=17)
    print(f"{kind}: {res_a}")
    assert res_a == res_b
    # the composition: model sampler -> upload -> the same decoders' device entries -> model score
    ex, ez = cm.sample(72, TRIALS, P, seed=17)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    want = np.zeros(6, dtype=np.int64)
    nc = [0, 0]
    for c0 in range(0, TRIALS, 1024):
        guesses = []
        for k, (dec, syn) in enumerate(((dec_hx, sx), (dec_hz, sz))):
            d_syn = torch.from_numpy(np.ascontiguousarray(syn[c0:c0 + 1024])).cuda()
            b = d_syn.shape[0]
            g = torch.empty((b, 72), dtype=torch.uint8, device="cuda")
            conv = torch.empty(b, dtype=torch.uint8, device="cuda")
            if kind == "bp":
                dec.decode_batch_device(d_syn, g, conv)
            else:
                dec.decode_batch_device(d_syn, g, conv, column0=c0)
            torch.cuda.synchronize()
            guesses.append(_np(g))
            nc[k] += int((_np(conv) == 0).sum())
        gz, gx = guesses                                # the decoder on Hx guesses the Z parts, the one on Hz the X parts
        want += cm.score(Hx, Hz, Lx, Lz, gx, gz, ex[c0:c0 + 1024], ez[c0:c0 + 1024])[1]
    assert res_a == ldpc.CSSTrialResult(TRIALS, int(want[1]), int(want[2]), int(want[3]), int(want[4]), int(want[5]), nc[0], nc[1])
    assert res_a.trials == TRIALS and res_a.logical_error_rate == want[3] / TRIALS
    dec_hx.close(); dec_hz.close()


def test_run_css_trials_refuses_decoders_that_are_no_pair(ldpc, gpu):
    dec_hx = ldpc.BeliefPropagationDecoder(_code("bb72")[0], 0.02, 5)
    dec_hz = ldpc.BeliefPropagationDecoder(_code("toy")[1], 0.02, 5)
    with pytest.raises(AssertionError, match="same number of bits"):
        ldpc.run_css_trials(dec_hx, dec_hz, 10, 0.03)
    dec_hx.close(); dec_hz.close()


# ---- arguments ------------------------------------------------------------------------------------------------------
def test_argument_validation_on_the_device_launches_nothing(ldpc, gpu):
    import ctypes

    import torch

    Hx, Hz, _, _ = _code("bb72")
    with pytest.raises(ldpc.LdpcError) as ei:
        ldpc.CSSTrials(Hx, Hz, logicals=False, kernel_variant=3)
    assert ei.value.status == 1
    t = _handle(ldpc, "bb72", 0)
    L, h = t._L, t._h
    fill = lambda cols: torch.full((4, cols), 0xEE, dtype=torch.uint8, device="cuda")   # noqa: E731
    ex, ez, gx, gz, sx, sz = fill(72), fill(72), fill(72), fill(72), fill(36), fill(36)
    counts = torch.full((6,), 7, dtype=torch.int64, device="cuda")
    P_ = lambda x: x.data_ptr()   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sample, synd, score = L.ldpc_css_trials_sample_device, L.ldpc_css_trials_syndromes_device, L.ldpc_css_trials_score_device
    # batch = 0: LDPC_OK (NULL pointers included), nothing touched
    assert sample(h, 0, 0, 0.1, 0.1, 0.1, 0, None, None, None, None, st) == 0
    assert synd(h, 0, None, None, None, None, st) == 0
    assert score(h, 0, None, None, None, None, None, None, st) == 0
    assert L.ldpc_css_trials_sample(h, 0, 0, 0.1, 0.1, 0.1, 0, None, None, None, None) == 0
    assert L.ldpc_css_trials_score(h, 0, None, None, None, None, None, None) == 0
    # negative batch, NULL required pointers, bad rates: LDPC_ERR_INVALID_ARGUMENT
    assert sample(h, -1, 0, 0.1, 0.1, 0.1, 0, P_(ex), P_(ez), P_(sx), P_(sz), st) == 1
    assert sample(h, 4, -1, 0.1, 0.1, 0.1, 0, P_(ex), P_(ez), P_(sx), P_(sz), st) == 1
    assert sample(h, 4, 0, 0.1, 0.1, 0.1, 0, None, P_(ez), P_(sx), P_(sz), st) == 1
    assert sample(h, 4, 0, 0.1, 0.1, 0.1, 0, P_(ex), None, P_(sx), P_(sz), st) == 1
    for rates in ((0.5, 0.5, 0.0), (float("nan"), 0.0, 0.0), (0.0, -0.1, 0.0), (0.0, 0.0, 1.0)):
        assert sample(h, 4, 0, *rates, 0, P_(ex), P_(ez), P_(sx), P_(sz), st) == 1
    assert synd(h, -1, P_(ex), P_(ez), P_(sx), P_(sz), st) == 1
    for k in range(4):
        args = [P_(ex), P_(ez), P_(sx), P_(sz)]
        args[k] = None
        assert synd(h, 4, *args, st) == 1
    assert score(h, -1, P_(gx), P_(gz), P_(ex), P_(ez), None, P_(counts), st) == 1
    for k in (0, 1, 2, 3, 5):
        args = [P_(gx), P_(gz), P_(ex), P_(ez), None, P_(counts)]
        args[k] = None
        assert score(h, 4, *args, st) == 1
    torch.cuda.synchronize()
    for x in (ex, ez, gx, gz, sx, sz):
        assert bool((x == 0xEE).all())
    assert _np(counts).tolist() == [7] * 6
    t.close()
