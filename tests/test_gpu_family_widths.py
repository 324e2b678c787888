"""The joint X/Z (Pauli) decoder, the flooding entries with per-syndrome priors and the layered schedule at the tile widths
their own suites do not reach, against the numpy models of their rules (tests/pauli_model.py, priors_model.py,
layered_model.py): equality in every element -- errors, flags, iteration counts, and the LLRs as bit patterns; the arithmetic
has no division and no transcendental function, so there is no tolerance.  The pattern of tests/test_gpu_minsum_tiles.py: a
table n -> (tier, S, max_iters, rate), a batch of two full tiles and a ragged one, a waterfall across the batch, and what
ran read back and asserted.  tests/test_tile_plan_cpu.py holds the rows (PAULI_TABLE, PRIORS_TABLE) against the planner.

  a. Pauli (pauli_kernels.hpp: `l = t & (S - 1)`, `q = t >> sh`, the `<< sh` of every state row): S = 16, 4, 2 and 1 on chip
     -- S = 1 under both LDS budgets -- and the unlimited tier chosen by size; S = 64, 32 and 8 run in tests/test_gpu_pauli.py
  b. the flooding priors entries (minsum_kernels.hpp: the block P behind syn at `(... + s S + 3) & ~3`, tile_plan.hpp
     ms_priors_offset): S = 64, 16, 8, 4, 2 and 1; at S = 2 and S = 1 with an odd number of checks, so that P starts 2 and 3
     padding bytes behind the syndrome bytes; the plain entry of the same handle, whose plan is another, before and after
  c. the layered schedule (layered_kernels.hpp) at S = 32, 8 and 1 through the floats entry with per-row priors

Model cost, measured on one CPU core each with three models running side by side: Pauli n = 6912, 4 iterations, 165 columns
6.5 s, n = 6144, 4 iterations, 7 columns 3.6 s; the three priors models of n = 6144, 5 iterations, together 6.6 s; layered
n = 6144, 5 iterations 4.0 s; every other shape below 3 s.  The iteration counts are chosen so that no model call exceeds
about 10 s; each result is computed once, shared, and never written to."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import priors_model as pm
from layered_model import LayeredMinSumModel
from minsum_model import MinSumModel, llr_of_probs
from pauli_model import PauliMinSumModel, pauli_priors
from test_gpu_minsum import _device as ms_device
from test_gpu_minsum import _same as ms_same
from test_gpu_minsum_tiles import MS_SHAPES, batch_of, ragged_prefix_of, tiles_of
from test_gpu_pauli import device_entry as pauli_device
from test_gpu_pauli import frozen
from test_gpu_pauli import same as pauli_same
from test_gpu_priors import _entry as priors_entry
from test_tile_plan_cpu import PAULI_TABLE, PRIORS_TABLE

pytestmark = pytest.mark.gpu
F = np.float32


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


def waterfall(conv, its, B, what):
    """Converged and unconverged rows, and at least three iteration counts where the batch has five rows."""
    assert 0 < conv.sum() < B, (what, int(conv.sum()), B)
    if B >= 5:
        assert len(set(its.tolist())) >= 3, (what, sorted(set(its.tolist())))


# ---- a. Pauli ---------------------------------------------------------------------------------------------------------------
# n -> (max_iters, rate): rate = the mean total Pauli probability of a qubit; row b is sampled at 0.1 ... 1.9 times the
# qubits' probabilities.  Picked with the model so that every batch is a waterfall (asserted below on the model's output).
PAULI_SHAPES = {192: (10, 0.06), 768: (10, 0.06), 1536: (8, 0.06), 3072: (6, 0.06), 6144: (4, 0.06), 6912: (4, 0.06)}


@functools.lru_cache(maxsize=None)
def pauli_case(n):
    """Hx and Hz (3,6)-regular over n qubits from different seeds (the sides do not commute: check=False), per-qubit
    (px, py, pz), batch_of(S) trials sampled qubit by qubit.  -> (Hx, Hz, probs, sx, sz, model output)."""
    ldpc = _ldpc()
    tier, S = PAULI_TABLE[n]
    iters, rate = PAULI_SHAPES[n]
    B = batch_of(S)
    Hx, Hz = ldpc.codes.parity_check_csc(n, 6, 3, seed=1), ldpc.codes.parity_check_csc(n, 6, 3, seed=2)
    assert Hx.shape == Hz.shape == (n // 2, n) and (Hx != Hz).nnz > 0
    rng = np.random.default_rng(n)
    probs = rate / 3.0 * rng.uniform(0.5, 1.5, (n, 3))
    scale = rng.permutation(np.linspace(0.1, 1.9, B))
    edges = np.cumsum(probs[None, :, :] * scale[:, None, None], axis=2)
    pauli = (rng.random((B, n, 1)) >= edges).sum(axis=2)                      # 0 = X, 1 = Y, 2 = Z, 3 = I
    ex, ez = (pauli <= 1).astype(np.uint8), ((pauli == 1) | (pauli == 2)).astype(np.uint8)
    sx, sz = ldpc.codes.syndromes_of(Hx, ez), ldpc.codes.syndromes_of(Hz, ex)
    priors = pauli_priors(probs)
    assert len(set(priors.ravel().tolist())) > n                                # lanes and qubits are distinguishable
    want = PauliMinSumModel(Hx, Hz, priors, iters).decode(sx, sz)
    frozen(sx, sz, *want)
    waterfall(want[2], want[3], B, f"pauli n {n}")
    return Hx, Hz, probs, sx, sz, want


@pytest.mark.parametrize("n", sorted(PAULI_SHAPES))
def test_pauli_at_the_widths_16_4_2_1_and_the_unlimited_tier_by_size(ldpc, gpu, n):
    """pauli_kernels.hpp, automatic selection: S = 16 (n = 192), 4 (768), 2 (1536), 1 under 79 KiB (3072), 1 under 159 KiB
    (6144: one workgroup a CU), and GLOBAL = true because nothing fits (6912).  The tier and the width are asserted BEFORE
    the decode; the whole batch (2 S + S / 2 + 5 columns), then its prefix of two full tiles and a ragged one."""
    tier, S = PAULI_TABLE[n]
    iters, _ = PAULI_SHAPES[n]
    Hx, Hz, probs, sx, sz, want = pauli_case(n)
    B = sx.shape[0]
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, iters, pauli_probs=probs, check=False)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0), (dec.info(), tier, S)
    what = f"pauli n {n} tier {tier} S {S}"
    pauli_same(pauli_device(dec, sx, sz), want, f"{what}, batch {B}")
    assert dec.tile_syndromes == S and dec.last_grid == tiles_of(B, S) >= 3
    Bp = ragged_prefix_of(S)
    assert Bp <= B and tiles_of(Bp, S) == 3 and (S == 1 or Bp % S != 0)
    pauli_same(pauli_device(dec, sx[:Bp], sz[:Bp]), want, f"{what}, batch {Bp}", slice(0, Bp))
    assert dec.last_grid == 3
    dec.close()


# ---- b. the flooding entries with per-syndrome priors -----------------------------------------------------------------------
# (n, extra) -> (max_iters, rate) for the rows of PRIORS_TABLE
PRIORS_SHAPES = {(72, 0): (10, 0.05), (192, 0): (10, 0.05), (384, 0): (10, 0.05), (768, 0): (10, 0.05), (1536, 1): (8, 0.05),
                 (3072, 1): (6, 0.05), (6144, 0): (5, 0.05)}


def regular_with_a_row_of_33(n, extra):
    """(3,6)-regular, and with `extra` one more check over the 33 bits 0, 3, 6, ..., 96 at the end."""
    H = _ldpc().codes.parity_check_csc(n, 6, 3)
    if extra:
        row = np.zeros((1, n), dtype=np.uint8)
        row[0, 0:99:3] = 1
        H = sp.csc_matrix(sp.vstack([sp.csr_matrix(H), sp.csr_matrix(row)]))
        H.sort_indices()
    deg = np.diff(sp.csr_matrix(H).indptr)
    assert H.shape == (n // 2 + extra, n) and (deg[:n // 2] == 6).all() and (not extra or deg[-1] == 33)
    return H


def errors_with_the_last_check_unmatched(H, e, S):
    """Flips one bit of the last check in every column that is the last lane of a full tile and has a 0 there: the entry
    nearest to the block behind the syndrome bytes is then set in every full tile."""
    M = sp.csr_matrix(H)
    s = M.shape[0]
    j = int(M.indices[M.indptr[s - 1]])
    e = e.copy()
    syn = _ldpc().codes.syndromes_of(H, e)
    for b in range(S - 1, e.shape[0], S):
        if syn[b, s - 1] == 0:
            e[b, j] ^= 1
    return e


@functools.lru_cache(maxsize=None)
def priors_case(n, extra):
    """-> dict: H, syn, shared prior, per-row priors (row b: the priors of the probabilities row b was sampled from),
    two tables and given bytes, and the three model outputs (plain, floats, given)."""
    ldpc = _ldpc()
    (_, S), _ = PRIORS_TABLE[(n, extra)]
    iters, rate = PRIORS_SHAPES[(n, extra)]
    B = batch_of(S)
    H = regular_with_a_row_of_33(n, extra)
    s = H.shape[0]
    rng = np.random.default_rng(n + extra)
    probs = rate * rng.uniform(0.5, 1.5, n)
    scale = rng.permutation(np.linspace(0.1, 1.9, B))
    row_probs = probs[None, :] * scale[:, None]
    e = errors_with_the_last_check_unmatched(H, (rng.random((B, n)) < row_probs).astype(np.uint8), S)
    syn = ldpc.codes.syndromes_of(H, e)
    assert all(syn[b, s - 1] == 1 for b in range(S - 1, B, S))                # the last byte of every full tile's syndrome block
    shared = llr_of_probs(probs)
    pri = llr_of_probs(row_probs)
    # distinct in every row and bit: a P row read from another lane or another bit gives another result
    assert all(len(set(pri[:, j].tolist())) == B for j in range(0, n, max(1, n // 64))) and all(len(set(r.tolist())) > n // 2 for r in pri)
    t0, t1 = llr_of_probs(0.5 * probs), llr_of_probs(np.minimum(3.0 * probs, 0.4))
    given = rng.integers(0, 256, size=(B, n), dtype=np.uint8)
    want = dict(plain=MinSumModel(H, shared, iters).decode(syn), floats=pm.PriorsMinSumModel(H, iters).decode(syn, pri),
                given=pm.PriorsMinSumModel(H, iters).decode(syn, pm.select_priors(given, t0, t1)))
    for x in (syn, shared, pri, t0, t1, given) + sum(want.values(), ()):
        x.setflags(write=False)
    waterfall(want["floats"][1], want["floats"][2], B, f"priors n {n}")
    assert any((want[a][3].view(np.int32) != want[b][3].view(np.int32)).any() for a, b in (("plain", "floats"), ("plain", "given")))
    return dict(H=H, syn=syn, shared=shared, pri=pri, t0=t0, t1=t1, given=given, want=want, iters=iters)


@pytest.mark.parametrize("n,extra", sorted(PRIORS_SHAPES), ids=[f"n{n}{'-odd-s' if x else ''}" for n, x in sorted(PRIORS_SHAPES)])
def test_flooding_priors_entries_at_every_width_with_the_plain_entry_around_them(ldpc, gpu, n, extra):
    """minsum_kernels.hpp with SRC != kMsPriorTable: the block P [n][S] starts at the word boundary behind syn [s][S].
    n = 1536 with the row of 33: s = 769, S = 2, s S % 4 == 2; n = 3072 with it: s = 1537, S = 1, s S % 4 == 1 -- P starts 2
    and 3 padding bytes behind the last syndrome byte, which is set in the last lane of every full tile; n = 6144: S = 1 with
    s % 4 == 0, inside the 159 KiB budget.  One handle: the plain entry (its own plan, asserted), the floats entry, the given
    entry, the plain entry again."""
    (ptier, S), (tier, S_plain) = PRIORS_TABLE[(n, extra)]
    c = priors_case(n, extra)
    H, syn, want = c["H"], c["syn"], c["want"]
    s, B = H.shape[0], syn.shape[0]
    assert ((s * S) % 4 != 0) == bool(extra) and (extra or n != 6144 or s % 4 == 0)
    if (n, extra) == (1536, 1):
        assert (s, S, (s * S) % 4) == (769, 2, 2)
    if (n, extra) == (3072, 1):
        assert (s, S, (s * S) % 4) == (1537, 1, 1)
    dec = ldpc.MinSumDecoder(H, None, c["iters"], channel_llr=c["shared"])
    dec.set_conditional_priors(c["t0"], c["t1"])
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes, info.last_grid) == (tier, S_plain, ptier, S, 0), info
    Bp = ragged_prefix_of(S)
    assert tiles_of(B, S) >= 3 and Bp <= B and tiles_of(Bp, S) == 3 and (S == 1 or Bp % S != 0)
    what = f"priors n {n} s {s} S {S}"
    ms_same(ms_device(dec, np.array(syn)), want["plain"], what + ", plain entry first")
    assert dec.info().last_grid == tiles_of(B, S_plain)
    ms_same(priors_entry(dec, syn, c["pri"], "priors"), want["floats"], what + ", floats")
    assert dec.info().last_grid == tiles_of(B, S)
    ms_same(priors_entry(dec, syn, c["given"], "given"), want["given"], what + ", given")
    assert dec.info().last_grid == tiles_of(B, S)
    for kind in ("floats", "given"):      # two full tiles and a ragged one
        extra_in = c["pri"] if kind == "floats" else c["given"]
        got = priors_entry(dec, syn[:Bp], extra_in[:Bp], "priors" if kind == "floats" else "given")
        ms_same(got, tuple(x[:Bp] for x in want[kind]), f"{what}, {kind}, batch {Bp}")
        assert dec.info().last_grid == 3
    ms_same(ms_device(dec, np.array(syn)), want["plain"], what + ", plain entry afterwards")
    info = dec.info()
    assert (info.last_grid, info.tile_syndromes, info.priors_tile_syndromes) == (tiles_of(B, S_plain), S_plain, S)
    dec.close()


# ---- c. the layered schedule ------------------------------------------------------------------------------------------------
LAYERED_SHAPES = {192: (32, 10), 768: (8, 10), 6144: (1, 5)}      # n of MS_SHAPES -> (S, max_iters)


@functools.lru_cache(maxsize=None)
def layered_case(n):
    ldpc = _ldpc()
    S, iters = LAYERED_SHAPES[n]
    assert MS_SHAPES[n][:2] == (1, S)
    B = batch_of(S)
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    rng = np.random.default_rng(n + 7)
    probs = 0.05 * rng.uniform(0.5, 1.5, n)
    row_probs = probs[None, :] * rng.permutation(np.linspace(0.1, 1.9, B))[:, None]
    syn = ldpc.codes.syndromes_of(H, (rng.random((B, n)) < row_probs).astype(np.uint8))
    pri = llr_of_probs(row_probs)
    model = pm.PriorsLayeredModel(H, iters)
    want = model.decode(syn, pri)
    shared = LayeredMinSumModel(H, pri[0], iters).decode(syn)
    frozen(syn, pri, *want)
    waterfall(want[1], want[2], B, f"layered n {n}")
    assert (shared[3][1:].view(np.int32) != want[3][1:].view(np.int32)).any()      # a row decoded with row 0's priors shows
    return H, syn, pri, model.K, iters, want


@pytest.mark.parametrize("n", sorted(LAYERED_SHAPES))
def test_layered_floats_entry_at_the_widths_32_8_and_1(ldpc, gpu, n):
    """layered_kernels.hpp with SRC != kMsPriorTable at S = 32, 8 and 1 (its own suite runs S = 64, 16, 4 and 2): the
    layered schedule keeps no priors block, so its priors plan is its plain plan."""
    S, _ = LAYERED_SHAPES[n]
    H, syn, pri, K, iters, want = layered_case(n)
    B = syn.shape[0]
    dec = ldpc.MinSumDecoder(H, 0.05, iters, schedule="layered")
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.priors_kernel, info.priors_tile_syndromes, info.layers) == (1, S, 1, S, K), info
    ms_same(priors_entry(dec, syn, pri, "priors"), want, f"layered n {n} S {S}, floats")
    assert dec.info().last_grid == tiles_of(B, S) >= 3
    Bp = ragged_prefix_of(S)
    assert Bp <= B and tiles_of(Bp, S) == 3 and (S == 1 or Bp % S != 0)
    ms_same(priors_entry(dec, syn[:Bp], pri[:Bp], "priors"), tuple(x[:Bp] for x in want), f"layered n {n} S {S}, floats, batch {Bp}")
    assert dec.info().last_grid == 3
    dec.close()
