"""Joint X/Z (Pauli) min-sum decoder on the GPU against the numpy model of its rule (tests/pauli_model.py): equality in
every element -- gx, gz, flags, iteration counts, and the three LLR planes as bit patterns.  The arithmetic has no
division and no transcendental function, so there is no tolerance.  What ran is read back and asserted (`.kernel`,
`.tile_syndromes`, `.last_grid`), so a case that misses its tier or width fails instead of passing on another path.
Every model result is computed once, shared, and never written to."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
from pauli_model import PauliMinSumModel, depolarizing_priors, pauli_priors

pytestmark = pytest.mark.gpu


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


# ---- entries and comparison -----------------------------------------------------------------------------------------------

def device_entry(dec, sx, sz, want_llr=True, want_iters=True):
    """-> (gx, gz, conv, iters | None, llr | None), every output buffer pre-filled with a value no decode writes."""
    import torch

    B = sx.shape[0]
    d_sx = torch.from_numpy(np.array(sx, dtype=np.uint8, order="C")).cuda()      # (a copy: the shared inputs are read-only)
    d_sz = torch.from_numpy(np.array(sz, dtype=np.uint8, order="C")).cuda()
    gx = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    gz = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, 3, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    dec.decode_batch_device(d_sx, d_sz, gx, gz, conv, llr, its)
    torch.cuda.synchronize()
    return (gx.cpu().numpy(), gz.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy() if want_iters else None,
            llr.cpu().numpy() if want_llr else None)


def host_entry(dec, sx, sz, want_llr=True):
    gx, gz, conv, llr, its = dec.decode_batch_host(sx, sz, want_llr=want_llr)
    assert (llr is None) == (not want_llr)
    return gx, gz, conv, its, llr


def same(got, want, what, idx=slice(None)):
    """got = (gx, gz, conv, iters | None, llr f64 | None) of an entry, want = the model's (gx, gz, conv, iters, G f32)."""
    gx, gz, conv, its, llr = got
    mgx, mgz, mconv, mits, mG = (x[idx] for x in want)
    assert gx.shape == mgx.shape and np.array_equal(gx, mgx), f"{what}: gx differs in {int((gx != mgx).any(axis=1).sum())} of {len(gx)} columns"
    assert gz.shape == mgz.shape and np.array_equal(gz, mgz), f"{what}: gz differs in {int((gz != mgz).any(axis=1).sum())} of {len(gz)} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ in columns {np.nonzero(conv != mconv)[0][:8].tolist()}"
    if its is not None:
        assert its.dtype == np.int32 and np.array_equal(its, mits), f"{what}: iteration counts differ in columns {np.nonzero(its != mits)[0][:8].tolist()}"
    if llr is not None:
        assert llr.dtype == np.float64 and llr.shape == mG.shape
        assert np.array_equal(llr.view(np.int64), mG.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


def tiles_of(B, S):
    return (B + S - 1) // S


def frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)


def waterfall(conv, its, B):
    """The batch has converged and unconverged columns and more than three iteration counts."""
    assert 0 < conv.sum() < B, (int(conv.sum()), B)
    assert len(set(its.tolist())) > 3, sorted(set(its.tolist()))


# ---- BB-72 ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bb72():
    Hx, Hz = _ldpc().codes.bivariate_bicycle_72_12_6()
    return sp.csc_matrix(np.asarray(Hx, dtype=np.uint8)), sp.csc_matrix(np.asarray(Hz, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def bb72_syndromes():
    """200 trials mixed from p = 0.01 / 0.03 / 0.06 (66 + 67 + 67), interleaved so that every tile holds all three."""
    Hx, Hz = bb72()
    parts = [cm.sample(72, k, p, seed=20 + i) for i, (k, p) in enumerate(((66, 0.01), (67, 0.03), (67, 0.06)))]
    ex, ez = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    order = np.random.default_rng(5).permutation(200)
    ex, ez = ex[order], ez[order]
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    frozen(sx, sz)
    return sx, sz


@functools.lru_cache(maxsize=None)
def bb72_case(alpha, max_iters=30, clip=1e6):
    """The decoder is built at p = 0.06 whatever a trial was sampled at."""
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, 0.06), max_iters, alpha=alpha, clip=clip).decode(sx, sz)
    frozen(*want)
    return want


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_bb72_equals_the_model(ldpc, gpu, alpha, variant):
    """1800 B a syndrome: S = 32 on chip by size, 64 in the unlimited tier.  Device and host entries, LLRs on and off."""
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = bb72_case(alpha)
    waterfall(want[2], want[3], 200)
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30, alpha=alpha, kernel_variant=variant)
    tier, S = (1, 32) if variant == 0 else (2, 64)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0) and (dec.n, dec.rows_x, dec.rows_z) == (72, 36, 36)
    assert np.array_equal(dec.prior_x.view(np.int32), depolarizing_priors(72, 0.06)[0].view(np.int32))
    what = f"BB-72 alpha {alpha} tier {tier}"
    same(device_entry(dec, sx, sz), want, what + ", device entry")
    assert dec.last_grid == tiles_of(200, S) and dec.info().device == 0
    same(device_entry(dec, sx, sz, want_llr=False, want_iters=False), want, what + ", device entry without LLRs and iteration counts")
    same(host_entry(dec, sx, sz), want, what + ", host entry")
    same(host_entry(dec, sx, sz, want_llr=False), want, what + ", host entry without LLRs")
    dec.close()
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_clamps(ldpc, gpu, variant):
    """clip = 2.0 at alpha = 1: below every prior (log(0.94 / 0.02) = 3.85), so every first b is clamped."""
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want, loose = bb72_case(1.0, clip=2.0), bb72_case(1.0)
    assert (want[4].view(np.int32) != loose[4].view(np.int32)).any(axis=(1, 2)).sum() > 100     # the clamp is exercised
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30, alpha=1.0, clip=2.0, kernel_variant=variant)
    same(device_entry(dec, sx, sz), want, f"BB-72 clip 2 tier {variant}")
    dec.close()


@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_bb72_max_iters_0_1_2(ldpc, gpu, max_iters):
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = bb72_case(0.75, max_iters=max_iters)
    if max_iters == 0:
        assert all(not x.any() for x in want)
    else:
        assert 0 < want[2].sum() < 200 and set(want[3].tolist()) == set(range(1, max_iters + 1))
    for variant in (1, 2):
        dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, max_iters, kernel_variant=variant)
        same(device_entry(dec, sx, sz), want, f"BB-72 max_iters {max_iters} tier {variant}")
        same(host_entry(dec, sx[:70], sz[:70]), want, f"BB-72 max_iters {max_iters} tier {variant}, host entry", slice(0, 70))
        dec.close()


@functools.lru_cache(maxsize=None)
def biased_case():
    """Per-qubit (px, py, pz), each uniform in (0.002, 0.08), six qubits where one Pauli is likelier than I (a negative
    prior LLR in one table each), trials sampled qubit by qubit from those probabilities."""
    Hx, Hz = bb72()
    rng = np.random.default_rng(21)
    probs = rng.uniform(0.002, 0.08, (72, 3))
    probs[[3, 40]] = [0.5, 0.1, 0.1]
    probs[[17, 55]] = [0.1, 0.55, 0.05]
    probs[[29, 71]] = [0.05, 0.1, 0.6]
    priors = pauli_priors(probs)
    assert all((priors[k] < 0).sum() == 2 for k in range(3)) and len(set(priors.ravel().tolist())) > 200
    r = rng.random((150, 72, 1))
    edges = np.cumsum(np.minimum(probs, 0.05), axis=1)[None, :, :]            # sampled gently: most columns converge
    pauli = (r >= edges).sum(axis=2)                                          # 0 = X, 1 = Y, 2 = Z, 3 = I
    ex, ez = (pauli <= 1).astype(np.uint8), ((pauli == 1) | (pauli == 2)).astype(np.uint8)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    want = PauliMinSumModel(Hx, Hz, priors, 25).decode(sx, sz)
    frozen(sx, sz, *want)
    return probs, sx, sz, want


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_per_qubit_priors_with_negative_llrs(ldpc, gpu, variant):
    Hx, Hz = bb72()
    probs, sx, sz, want = biased_case()
    waterfall(want[2], want[3], 150)
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, 25, pauli_probs=probs, kernel_variant=variant)
    assert (dec.prior_x < 0).any() and (dec.prior_y < 0).any() and (dec.prior_z < 0).any()
    same(device_entry(dec, sx, sz), want, f"BB-72 biased priors tier {variant}")
    dec.close()


def test_bb72_a_handle_used_twice(ldpc, gpu):
    """Three calls on one handle, of other sizes and other columns: the state a tile finds is what the call before left."""
    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = bb72_case(0.75)
    for variant in (1, 2):
        dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30, kernel_variant=variant)
        for lo, hi in ((100, 200), (0, 200), (37, 70)):
            same(device_entry(dec, sx[lo:hi], sz[lo:hi]), want, f"tier {variant}, columns {lo}:{hi}", slice(lo, hi))
            assert dec.last_grid == tiles_of(hi - lo, dec.tile_syndromes)
        same(host_entry(dec, sx[5:6], sz[5:6]), want, f"tier {variant}, one column through the host entry", slice(5, 6))
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_bb72_more_tiles_than_resident_workgroups(ldpc, gpu, variant):
    """Slot reuse with no knob: the 200 known syndromes repeated with a roll of 13 per repetition, so that equal syndromes
    sit in other lanes and tiles, S (4 CUs + 1) + 5 of them -- more tiles than a device can host workgroups of 8 or 16
    waves (at most 4 and 2 a CU).  The grid must come out smaller than the tile count."""
    import torch

    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    want = bb72_case(0.75)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30, kernel_variant=variant)
    S = dec.tile_syndromes
    assert (dec.kernel, S) == ((1, 32) if variant == 1 else (2, 64))
    B = S * (4 * cus + 1) + 5
    b = np.arange(B)
    idx = (b + 13 * (b // 200)) % 200
    got = device_entry(dec, sx[idx], sz[idx])
    print(f"tier {variant}: {cus} CUs, batch {B}, tiles {tiles_of(B, S)}, last_grid {dec.last_grid}")
    assert 0 < dec.last_grid < tiles_of(B, S), (dec.info(), B)
    same(got, want, f"tier {variant}, batch {B}", idx)
    dec.close()


# ---- other widths -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def product_case(kind):
    """"small": the hypergraph product of two 3-bit repetition checks, n = 13, 308 B a syndrome: S = 64 on chip.
    "large": that of two (12, 4, 3) Gallager matrices, n = 225, 5472 B a syndrome: S = 8.  130 trials each."""
    ldpc = _ldpc()
    if kind == "small":
        rep = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
        Hx, Hz = ldpc.codes.hypergraph_product(rep, rep)
        p, iters, S = 0.12, 12, 64
    else:
        H = ldpc.codes.parity_check_csc(12, 4, 3)
        Hx, Hz = ldpc.codes.hypergraph_product(H, H)
        p, iters, S = 0.04, 12, 8
    n = Hx.shape[1]
    ex, ez = cm.sample(n, 130, p, seed=4)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    want = PauliMinSumModel(Hx, Hz, depolarizing_priors(n, p), iters).decode(sx, sz)
    frozen(sx, sz, *want)
    return Hx, Hz, p, iters, S, sx, sz, want


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("kind", ["small", "large"])
def test_hypergraph_products_at_batch_130_and_1(ldpc, gpu, kind, variant):
    """S = 64 and S = 8 on chip by size, and the unlimited tier: batch 130 ends in a ragged tile in all of them; batch 1."""
    Hx, Hz, p, iters, S, sx, sz, want = product_case(kind)
    assert Hx.shape[1] == (13 if kind == "small" else 225)
    assert 0 < want[2].sum() < 130 and len(set(want[3].tolist())) >= 3
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, p, iters, kernel_variant=variant)
    tier, S = (1, S) if variant == 0 else (2, 64)
    assert (dec.kernel, dec.tile_syndromes) == (tier, S) and 130 % S != 0
    what = f"hypergraph product n {dec.n} tier {tier} S {S}"
    same(device_entry(dec, sx, sz), want, what + ", batch 130")
    assert dec.last_grid == tiles_of(130, S)
    same(host_entry(dec, sx, sz), want, what + ", batch 130, host entry")
    same(device_entry(dec, sx[129:], sz[129:]), want, what + ", batch 1", slice(129, 130))
    assert dec.last_grid == 1
    dec.close()


# ---- record forms, empty nodes -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wide_row_case(n):
    """Hx = one all-ones row over n qubits (n = 40: the 5-word record; n = 70: one word per edge), Hz = the pairs
    (2k, 2k + 1) (4-word records); every pair overlaps the row in two qubits, so the sides commute.  A syndrome takes
    4 (80 + 5 + 80) + 21 = 681 B at n = 40 (S = 64 on chip) and 4 (140 + 70 + 140) + 36 = 1436 B at n = 70 (64 of them
    are 91904 B > 79 KiB: S = 32)."""
    Hx = sp.csc_matrix(np.ones((1, n), dtype=np.uint8))
    Hz = sp.csc_matrix((np.ones(n, dtype=np.uint8), (np.arange(n) // 2, np.arange(n))), shape=(n // 2, n))
    ex, ez = cm.sample(n, 90, 0.05, seed=n)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    rng = np.random.default_rng(n)
    probs = rng.uniform(0.01, 0.08, (n, 3))                       # per-qubit priors: the minima of the wide row are distinct
    want = PauliMinSumModel(Hx, Hz, pauli_priors(probs), 8).decode(sx, sz)
    frozen(sx, sz, *want)
    return Hx, Hz, probs, sx, sz, want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", [40, 70])
def test_record_forms_of_a_wide_row(ldpc, gpu, n, variant):
    Hx, Hz, probs, sx, sz, want = wide_row_case(n)
    assert 0 < want[2].sum() < 90 and len(set(want[3].tolist())) >= 2
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, 8, pauli_probs=probs, kernel_variant=variant)
    assert dec.kernel == variant and dec.tile_syndromes == (32 if (n, variant) == (70, 1) else 64)
    same(device_entry(dec, sx, sz), want, f"all-ones row over {n} qubits, tier {variant}")
    assert dec.last_grid == tiles_of(90, dec.tile_syndromes)
    dec.close()


@functools.lru_cache(maxsize=None)
def empty_nodes_case():
    """n = 8.  Hx: the row (0, 1, 2, 3) and an empty row.  Hz: the pairs (0, 1), (2, 3), an empty row, the pair (4, 5).
    Qubits 4 and 5 are in checks of one side only, qubits 6 and 7 in no check; qubit 7 has negative priors.  The
    syndromes are all 2^6 combinations with the entries of the empty checks taken from a counter: a set entry of an empty
    check can never be matched."""
    Hx = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [0] * 8], dtype=np.uint8)
    Hz = np.array([[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0], [0] * 8, [0, 0, 0, 0, 1, 1, 0, 0]], dtype=np.uint8)
    bits = (np.arange(64)[:, None] >> np.arange(6)[None, :]) & 1
    sx, sz = bits[:, :2].astype(np.uint8), bits[:, 2:].astype(np.uint8)
    sx[:, 1] *= 3                                                # an entry that is not 0 counts as 1
    probs = np.random.default_rng(8).uniform(0.02, 0.1, (8, 3))
    probs[7] = [0.4, 0.3, 0.2]
    want = PauliMinSumModel(Hx, Hz, pauli_priors(probs), 6).decode(sx, sz)
    frozen(sx, sz, *want)
    return Hx, Hz, probs, sx, sz, want


@pytest.mark.parametrize("variant", [1, 2])
def test_empty_checks_and_isolated_qubits(ldpc, gpu, variant):
    Hx, Hz, probs, sx, sz, want = empty_nodes_case()
    gx, gz, conv, its, G = want
    empty_set = (sx[:, 1] != 0) | (sz[:, 2] != 0)
    assert not conv[empty_set].any() and conv[~empty_set].any() and (gx[:, 7] | gz[:, 7]).all() and not gx[:, 6].any()
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, 6, pauli_probs=probs, kernel_variant=variant)
    same(device_entry(dec, sx, sz), want, f"empty nodes, tier {variant}")
    same(host_entry(dec, sx, sz), want, f"empty nodes, tier {variant}, host entry")
    dec.close()


# ---- the trials driver -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trials_case():
    """1,000 trials of BB-72 at depolarizing 0.06, seed 9: css_trials_model sample -> PauliMinSumModel -> model score."""
    ldpc = _ldpc()
    Hx, Hz = bb72()
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
    ex, ez = cm.sample(72, 1000, 0.06, seed=9)
    sx, sz = cm.syndromes(Hx, Hz, ex, ez)
    gx, gz, conv, its, _ = PauliMinSumModel(Hx, Hz, depolarizing_priors(72, 0.06), 30).decode(sx, sz)
    _, counts = cm.score(Hx, Hz, Lx, Lz, gx, gz, ex, ez)
    nc = int((conv == 0).sum())
    return ldpc.CSSTrialResult(trials=int(counts[0]), block_errors=int(counts[1]), syndrome_mismatches=int(counts[2]),
                               logical_errors=int(counts[3]), logical_x_errors=int(counts[4]), logical_z_errors=int(counts[5]),
                               not_converged_hx=nc, not_converged_hz=nc)


def test_run_css_joint_trials_equals_the_model_loop(ldpc, gpu):
    Hx, Hz = bb72()
    want = trials_case()
    assert want.trials == 1000 and 0 < want.logical_errors < 1000 and 0 < want.not_converged_hx < 1000
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30)
    a = ldpc.run_css_joint_trials(dec, 1000, 0.06, batch=256, seed=9)
    b = ldpc.run_css_joint_trials(dec, 1000, 0.06, batch=1000, seed=9)
    assert a == b == want, (a, b, want)
    assert a.not_converged_hx == a.not_converged_hz
    assert ldpc.run_css_joint_trials(dec, 0, 0.06).trials == 0
    dec.close()
