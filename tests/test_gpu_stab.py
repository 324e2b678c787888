"""Stabilizer (non-CSS) min-sum decoder on the GPU against the numpy model of its rule (tests/stab_model.py): equality in
every element -- gx, gz, flags, iteration counts, and the three LLR planes as bit patterns.  The arithmetic has no
division and no transcendental function, so there is no tolerance.  What ran is read back and asserted (`.kernel`,
`.tile_syndromes`, `.last_grid`), so a case that misses its tier or width fails instead of passing on another path.
Every batch holds converged and unconverged columns.  Every model result is computed once, shared, and never written to.

Tested elsewhere: every tile width (S = 64 ... 1, both LDS budgets, the largest on-chip state, the unlimited tier by size) in
tests/test_gpu_stab_widths.py; the record forms at degrees 31, 32, 33, 63, 64 and 65 and the zeros and ties of the decision
in tests/test_gpu_stab_boundaries.py (CPU twin: tests/test_stab_boundaries_cpu.py); random graphs in the leg `stab` of
tools/fuzz_models.py (tests/test_gpu_fuzz_models.py)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import css_trials_model as cm
import trials_model as tm
from pauli_model import depolarizing_priors, pauli_priors
from stab_model import StabMinSumModel, symplectic_syndromes
from test_gpu_pauli import bb72, bb72_syndromes, frozen, same, tiles_of, waterfall

pytestmark = pytest.mark.gpu


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


# ---- entries --------------------------------------------------------------------------------------------------------------

def device_entry(dec, s, want_llr=True, want_iters=True):
    """-> (gx, gz, conv, iters | None, llr | None), every output buffer pre-filled with a value no decode writes."""
    import torch

    B = s.shape[0]
    d_s = torch.from_numpy(np.array(s, dtype=np.uint8, order="C")).cuda()      # (a copy: the shared inputs are read-only)
    gx = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    gz = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, 3, dec.n), 7.0, dtype=torch.float64, device="cuda") if want_llr else None
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    dec.decode_batch_device(d_s, gx, gz, conv, llr, its)
    torch.cuda.synchronize()
    return (gx.cpu().numpy(), gz.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy() if want_iters else None,
            llr.cpu().numpy() if want_llr else None)


def host_entry(dec, s, want_llr=True):
    gx, gz, conv, llr, its = dec.decode_batch_host(s, want_llr=want_llr)
    assert (llr is None) == (not want_llr)
    return gx, gz, conv, its, llr


def mixed(conv, B):
    assert 0 < conv.sum() < B, (int(conv.sum()), B)


# ---- the deformed BB-72: all three edge types ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def deformed():
    Hx, Hz = bb72()
    Sx, Sz = _ldpc().codes.clifford_deform(Hx, Hz, np.random.default_rng(7).integers(0, 6, 72))
    A, B = Sx.toarray(), Sz.toarray()
    assert (int((A & ~B & 1).sum()), int((B & ~A & 1).sum()), int((A & B).sum())) == (144, 150, 138)
    return Sx, Sz


@functools.lru_cache(maxsize=None)
def deformed_syndromes():
    """The 200 mixed trials of test_gpu_pauli.bb72_syndromes (0.01 / 0.03 / 0.06), the same errors, mapped through the
    symplectic syndrome of the deformed code."""
    Sx, Sz = deformed()
    parts = [cm.sample(72, k, p, seed=20 + i) for i, (k, p) in enumerate(((66, 0.01), (67, 0.03), (67, 0.06)))]
    ex, ez = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    order = np.random.default_rng(5).permutation(200)
    ex, ez = ex[order], ez[order]
    Hx, Hz = bb72()
    assert np.array_equal(cm.syndromes(Hx, Hz, ex, ez)[0], bb72_syndromes()[0])       # the errors behind bb72_syndromes()
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    frozen(s)
    return s


@functools.lru_cache(maxsize=None)
def deformed_case(alpha, max_iters=30, clip=1e6):
    """The decoder is built at p = 0.06 whatever a trial was sampled at."""
    Sx, Sz = deformed()
    want = StabMinSumModel(Sx, Sz, depolarizing_priors(72, 0.06), max_iters, alpha=alpha, clip=clip).decode(deformed_syndromes())
    frozen(*want)
    return want


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_deformed_bb72_equals_the_model(ldpc, gpu, alpha, variant):
    """2088 B a syndrome: S = 32 on chip by size, 64 in the unlimited tier.  Device and host entries, LLRs on and off."""
    Sx, Sz = deformed()
    s = deformed_syndromes()
    want = deformed_case(alpha)
    waterfall(want[2], want[3], 200)
    if alpha == 0.75:
        assert int(want[2].sum()) == 198 and len(set(want[3].tolist())) == 13
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30, alpha=alpha, kernel_variant=variant)
    tier, S = (1, 32) if variant == 0 else (2, 64)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0) and (dec.n, dec.rows) == (72, 72)
    assert np.array_equal(dec.prior_x.view(np.int32), depolarizing_priors(72, 0.06)[0].view(np.int32))
    what = f"deformed BB-72 alpha {alpha} tier {tier}"
    same(device_entry(dec, s), want, what + ", device entry")
    assert dec.last_grid == tiles_of(200, S) and dec.info().device == 0
    same(device_entry(dec, s, want_llr=False, want_iters=False), want, what + ", device entry without LLRs and iteration counts")
    same(host_entry(dec, s), want, what + ", host entry")
    same(host_entry(dec, s, want_llr=False), want, what + ", host entry without LLRs")
    dec.close()
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_deformed_bb72_clamps(ldpc, gpu, variant):
    """clip = 2.0 at alpha = 1: below every prior (log(0.94 / 0.02) = 3.85), so every first b is clamped."""
    Sx, Sz = deformed()
    want, loose = deformed_case(1.0, clip=2.0), deformed_case(1.0)
    mixed(want[2], 200)
    assert (want[4].view(np.int32) != loose[4].view(np.int32)).any(axis=(1, 2)).sum() > 100     # the clamp is exercised
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30, alpha=1.0, clip=2.0, kernel_variant=variant)
    same(device_entry(dec, deformed_syndromes()), want, f"deformed BB-72 clip 2 tier {variant}")
    dec.close()


@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_deformed_bb72_max_iters_0_1_2(ldpc, gpu, max_iters):
    Sx, Sz = deformed()
    s = deformed_syndromes()
    want = deformed_case(0.75, max_iters=max_iters)
    if max_iters == 0:
        assert all(not x.any() for x in want)
    else:
        assert 0 < want[2].sum() < 200 and set(want[3].tolist()) == set(range(1, max_iters + 1))
    for variant in (1, 2):
        dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, max_iters, kernel_variant=variant)
        same(device_entry(dec, s), want, f"deformed BB-72 max_iters {max_iters} tier {variant}")
        same(host_entry(dec, s[:70]), want, f"deformed BB-72 max_iters {max_iters} tier {variant}, host entry", slice(0, 70))
        dec.close()


@functools.lru_cache(maxsize=None)
def biased_case():
    """Per-qubit (px, py, pz), each uniform in (0.002, 0.08), six qubits where one Pauli is likelier than I (a negative
    prior LLR in one table each), trials sampled qubit by qubit from those probabilities."""
    Sx, Sz = deformed()
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
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    want = StabMinSumModel(Sx, Sz, priors, 25).decode(s)
    frozen(s, *want)
    return probs, s, want


@pytest.mark.parametrize("variant", [1, 2])
def test_deformed_bb72_per_qubit_priors_with_negative_llrs(ldpc, gpu, variant):
    Sx, Sz = deformed()
    probs, s, want = biased_case()
    mixed(want[2], 150)
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, None, 25, pauli_probs=probs, kernel_variant=variant)
    assert (dec.prior_x < 0).any() and (dec.prior_y < 0).any() and (dec.prior_z < 0).any()
    same(device_entry(dec, s), want, f"deformed BB-72 biased priors tier {variant}")
    dec.close()


def test_deformed_bb72_a_handle_used_three_times(ldpc, gpu):
    """Three calls on one handle, of other sizes and other columns: the state a tile finds is what the call before left."""
    Sx, Sz = deformed()
    s = deformed_syndromes()
    want = deformed_case(0.75)
    for variant in (1, 2):
        dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30, kernel_variant=variant)
        for lo, hi in ((100, 200), (0, 200), (163, 200)):       # (columns 194 and 199 do not converge)
            mixed(want[2][lo:hi], hi - lo)
            same(device_entry(dec, s[lo:hi]), want, f"tier {variant}, columns {lo}:{hi}", slice(lo, hi))
            assert dec.last_grid == tiles_of(hi - lo, dec.tile_syndromes)
        same(host_entry(dec, s[190:196]), want, f"tier {variant}, six columns through the host entry", slice(190, 196))
        dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_deformed_bb72_more_tiles_than_resident_workgroups(ldpc, gpu, variant):
    """Slot reuse with no knob: the 200 known syndromes repeated with a roll of 13 per repetition, so that equal syndromes
    sit in other lanes and tiles, S (4 CUs + 1) + 5 of them -- more tiles than a device can host workgroups of 8 or 16
    waves.  The grid must come out smaller than the tile count."""
    import torch

    Sx, Sz = deformed()
    s = deformed_syndromes()
    want = deformed_case(0.75)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30, kernel_variant=variant)
    S = dec.tile_syndromes
    assert (dec.kernel, S) == ((1, 32) if variant == 1 else (2, 64))
    B = S * (4 * cus + 1) + 5
    b = np.arange(B)
    idx = (b + 13 * (b // 200)) % 200
    got = device_entry(dec, s[idx])
    print(f"tier {variant}: {cus} CUs, batch {B}, tiles {tiles_of(B, S)}, last_grid {dec.last_grid}")
    assert 0 < dec.last_grid < tiles_of(B, S), (dec.info(), B)
    same(got, want, f"tier {variant}, batch {B}", idx)
    dec.close()


# ---- a CSS input equals the Pauli decoder -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 2])
def test_css_input_equals_the_pauli_decoder_in_every_bit(ldpc, gpu, variant):
    """BB-72 as [Hx; 0], [0; Hz]: the outputs equal those of PauliMinSumDecoder on the same GPU, and the model's."""
    import test_gpu_pauli as tp

    Hx, Hz = bb72()
    sx, sz = bb72_syndromes()
    Sx, Sz = ldpc.codes.clifford_deform(Hx, Hz, np.zeros(72, dtype=np.int64))
    s = np.concatenate([sx, sz], axis=1)
    want = tp.bb72_case(0.75)                                   # PauliMinSumModel
    waterfall(want[2], want[3], 200)
    mine = StabMinSumModel(Sx, Sz, depolarizing_priors(72, 0.06), 30).decode(s)
    for a, b in zip(mine, want):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30, kernel_variant=variant)
    ref = ldpc.PauliMinSumDecoder(Hx, Hz, 0.06, 30, kernel_variant=variant)
    assert (dec.kernel, dec.tile_syndromes) == (ref.kernel, ref.tile_syndromes) == ((1, 32) if variant == 0 else (2, 64))
    got, got_ref = device_entry(dec, s), tp.device_entry(ref, sx, sz)
    for a, b, name in zip(got, got_ref, ("gx", "gz", "converged", "iters", "llr")):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                     b.view(np.int64) if b.dtype == np.float64 else b), name
    same(got, want, f"CSS input, tier {dec.kernel}")
    dec.close()
    ref.close()


# ---- the five-qubit code ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def five_case(alpha):
    Fx, Fz = _ldpc().codes.five_qubit_code()
    syn = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    want = StabMinSumModel(Fx, Fz, depolarizing_priors(5, 0.03), 10, alpha=alpha).decode(syn)
    frozen(syn, *want)
    return syn, want


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_five_qubit_code_all_16_syndromes(ldpc, gpu, alpha, variant):
    """A ragged tile of 16 in S = 64; 15 (alpha 0.75) and 9 (alpha 1.0) of the 16 converge."""
    syn, want = five_case(alpha)
    assert int(want[2].sum()) == (15 if alpha == 0.75 else 9)
    dec = ldpc.StabilizerMinSumDecoder.from_paulis(["XZZXI", "IXZZX", "XIXZZ", "ZXIXZ"], 0.03, 10, alpha=alpha, kernel_variant=variant)
    assert (dec.kernel, dec.tile_syndromes, dec.n, dec.rows) == (1 if variant == 0 else 2, 64, 5, 4)
    same(device_entry(dec, syn), want, f"five-qubit code alpha {alpha} tier {dec.kernel}")
    assert dec.last_grid == 1
    same(host_entry(dec, syn), want, f"five-qubit code alpha {alpha} tier {dec.kernel}, host entry")
    dec.close()


# ---- other widths -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def width_case(kind):
    """"xzzx": xzzx_surface_code(5) at (0.004, 0.004, 0.10), n = 41, 1172 B a syndrome: S = 64 on chip.  "hgp": the
    hypergraph product of two (12, 4, 3) Gallager matrices deformed with default_rng(11), n = 225, 6372 B a syndrome:
    S = 8, depolarizing 0.04.  130 trials of seed 4 and 12 iterations each."""
    ldpc = _ldpc()
    if kind == "xzzx":
        Sx, Sz = ldpc.codes.xzzx_surface_code(5)
        p, S, conv = (0.004, 0.004, 0.10), 64, 97
    else:
        H = ldpc.codes.parity_check_csc(12, 4, 3)
        Hx, Hz = ldpc.codes.hypergraph_product(H, H)
        Sx, Sz = ldpc.codes.clifford_deform(Hx, Hz, np.random.default_rng(11).integers(0, 6, 225))
        p, S, conv = 0.04, 8, 58
    n = Sx.shape[1]
    ex, ez = cm.sample(n, 130, p, seed=4)
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    want = StabMinSumModel(Sx, Sz, depolarizing_priors(n, p), 12).decode(s)
    assert int(want[2].sum()) == conv
    frozen(s, *want)
    return Sx, Sz, p, S, s, want


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("kind", ["xzzx", "hgp"])
def test_other_widths_at_batch_130_and_1(ldpc, gpu, kind, variant):
    """S = 64 and S = 8 on chip by size, and the unlimited tier: batch 130 ends in a ragged tile in all of them; batch 1."""
    Sx, Sz, p, S, s, want = width_case(kind)
    assert Sx.shape[1] == (41 if kind == "xzzx" else 225)
    mixed(want[2], 130)
    assert len(set(want[3].tolist())) >= 3
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, p, 12, kernel_variant=variant)
    tier, S = (1, S) if variant == 0 else (2, 64)
    assert (dec.kernel, dec.tile_syndromes) == (tier, S) and 130 % S != 0
    what = f"{kind} n {dec.n} tier {tier} S {S}"
    same(device_entry(dec, s), want, what + ", batch 130")
    assert dec.last_grid == tiles_of(130, S)
    same(host_entry(dec, s), want, what + ", batch 130, host entry")
    same(device_entry(dec, s[129:]), want, what + ", batch 1", slice(129, 130))
    assert dec.last_grid == 1
    dec.close()


# ---- record forms, empty nodes -------------------------------------------------------------------------------------------------

_TYPE_BITS = (1, 3, 2)   # X, Y, Z as (X part) | (Z part) << 1


@functools.lru_cache(maxsize=None)
def wide_row_case(n):
    """Row 0 over all n qubits with types cycling X, Y, Z (n = 40: the 5-word record; n = 70: one word per edge), rows
    1 + k over the pairs (2k, 2k + 1) with types (k mod 3, (k + 1) mod 3) (4-word records).  The rows need not commute:
    the library does not look.  A syndrome takes 4 (120 + 85) + 21 = 841 B at n = 40 (S = 64 on chip) and
    4 (210 + 210) + 36 = 1716 B at n = 70 (64 of them are 109824 B > 79 KiB: S = 32)."""
    T = np.zeros((1 + n // 2, n), dtype=np.int64)
    T[0] = [_TYPE_BITS[j % 3] for j in range(n)]
    for k in range(n // 2):
        T[1 + k, 2 * k], T[1 + k, 2 * k + 1] = _TYPE_BITS[k % 3], _TYPE_BITS[(k + 1) % 3]
    Sx, Sz = sp.csc_matrix((T & 1).astype(np.uint8)), sp.csc_matrix((T >> 1).astype(np.uint8))
    ex, ez = cm.sample(n, 90, 0.05, seed=n)
    s = symplectic_syndromes(Sx, Sz, ex, ez)
    probs = np.random.default_rng(n).uniform(0.01, 0.08, (n, 3))      # per-qubit priors: the minima of the wide row are distinct
    want = StabMinSumModel(Sx, Sz, pauli_priors(probs), 8).decode(s)
    assert int(want[2].sum()) == {40: 41, 70: 29}[n]
    frozen(s, *want)
    return Sx, Sz, probs, s, want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", [40, 70])
def test_record_forms_of_a_wide_row(ldpc, gpu, n, variant):
    Sx, Sz, probs, s, want = wide_row_case(n)
    mixed(want[2], 90)
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, None, 8, pauli_probs=probs, kernel_variant=variant, check=False)
    assert dec.kernel == variant and dec.tile_syndromes == (32 if (n, variant) == (70, 1) else 64)
    same(device_entry(dec, s), want, f"wide row over {n} qubits, tier {variant}")
    assert dec.last_grid == tiles_of(90, dec.tile_syndromes)
    dec.close()


@functools.lru_cache(maxsize=None)
def empty_nodes_case():
    """n = 8, r = 5.  Row 0: X Y Z X on qubits 0 .. 3; row 1 empty; row 2: Z Z on (0, 1); row 3 empty; row 4: Y X on (4, 5).
    Qubits 6 and 7 are in no check; qubit 7 has negative priors.  The syndromes are all 2^5 combinations; a set entry of an
    empty check can never be matched; the entries of row 3 are 3 where set (an entry that is not 0 counts as 1)."""
    Sx, Sz = _ldpc().codes.paulis_to_symplectic(["XYZXIIII", "IIIIIIII", "ZZIIIIII", "IIIIIIII", "IIIIYXII"])
    s = ((np.arange(32)[:, None] >> np.arange(5)[None, :]) & 1).astype(np.uint8)
    s[:, 3] *= 3
    probs = np.random.default_rng(8).uniform(0.02, 0.1, (8, 3))
    probs[7] = [0.4, 0.3, 0.2]
    want = StabMinSumModel(Sx, Sz, pauli_priors(probs), 6).decode(s)
    frozen(s, *want)
    return Sx, Sz, probs, s, want


@pytest.mark.parametrize("variant", [1, 2])
def test_empty_checks_and_isolated_qubits(ldpc, gpu, variant):
    Sx, Sz, probs, s, want = empty_nodes_case()
    gx, gz, conv, its, G = want
    empty_set = (s[:, 1] != 0) | (s[:, 3] != 0)
    assert not conv[empty_set].any() and conv[~empty_set].any() and (gx[:, 7] | gz[:, 7]).all() and not gx[:, 6].any()
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, None, 6, pauli_probs=probs, kernel_variant=variant, check=False)
    same(device_entry(dec, s), want, f"empty nodes, tier {variant}")
    same(host_entry(dec, s), want, f"empty nodes, tier {variant}, host entry")
    dec.close()


# ---- the trials driver -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trials_case():
    """1,000 trials of the deformed BB-72 at depolarizing 0.06, seed 9: css_trials_model sample -> StabMinSumModel -> the
    binary model score over [Sz | Sx] with the logical rows [LSz | LSx]."""
    ldpc = _ldpc()
    Sx, Sz = deformed()
    LSx, LSz = ldpc.codes.stabilizer_logicals(Sx, Sz)
    ex, ez = cm.sample(72, 1000, 0.06, seed=9)
    gx, gz, conv, its, _ = StabMinSumModel(Sx, Sz, depolarizing_priors(72, 0.06), 30).decode(symplectic_syndromes(Sx, Sz, ex, ez))
    _, counts = tm.score(sp.csr_matrix(sp.hstack([Sz, Sx])), np.concatenate([LSz, LSx], axis=1), np.concatenate([gx, gz], axis=1),
                         np.concatenate([ex, ez], axis=1))
    return ldpc.TrialResult(trials=int(counts[0]), block_errors=int(counts[1]), syndrome_mismatches=int(counts[2]),
                            logical_errors=int(counts[3]), not_converged=int((conv == 0).sum()))


def test_run_stabilizer_trials_equals_the_model_loop(ldpc, gpu):
    Sx, Sz = deformed()
    want = trials_case()
    assert want.trials == 1000 and 0 < want.logical_errors < 1000 and 0 < want.not_converged < 1000
    dec = ldpc.StabilizerMinSumDecoder(Sx, Sz, 0.06, 30)
    a = ldpc.run_stabilizer_trials(dec, 1000, 0.06, batch=256, seed=9)
    b = ldpc.run_stabilizer_trials(dec, 1000, 0.06, batch=1000, seed=9)
    assert a == b == want, (a, b, want)
    zero = ldpc.run_stabilizer_trials(dec, 0, 0.06)
    assert zero == ldpc.TrialResult(0, 0, 0, 0, 0)
    dec.close()
