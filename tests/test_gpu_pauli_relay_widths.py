"""The Pauli relay min-sum kernel (pauli_relay_kernels.hpp) at EVERY tile width, under both LDS budgets and in the unlimited
tier by size, against the numpy model of its rule (tests/pauli_relay_model.py): equality in every element -- gx, gz, flags,
iteration counts, solution counts, and the three LLR planes as bit patterns; no tolerance.  The pattern of
tests/test_gpu_decim_widths.py.

The kernel indexes every row of G, M, the records, best and the syndromes by `<< sh` with `l = t & (S - 1)`, `q = t >> sh`,
`Q = T >> sh`: at S = 64 a lane is shared by 8 threads of the on-chip kernel, at S = 1 by all 512, and they meet in the one
`atomicAdd` on `sh_w[l]` (the weight of a solution) and in the words of `best`.  tests/test_gpu_pauli_relay.py runs S = 16 and
the forced unlimited tier only.

The graph is a small CSS core -- the hypergraph product of two 3-bit repetition checks, n = 13, 6 + 6 checks -- padded with
isolated qubits and empty checks until a lane has the size of a row of WIDTH_TABLE (tests/test_pauli_relay_cpu.py holds the
table against the planner).  The models loop over the edges in Python, so their cost stays that of the core: well below a
second a row.  An isolated qubit is no idle ballast: its three posteriors follow M = g0 + gamma M through every iteration and
leg, its decision enters every weight and both bit planes of best, and its priors have both signs.  Every case asserts ON THE
MODEL, before anything touches the GPU, that its batch holds converged and unconverged lanes, lanes that stop in different
legs, and every solution count.  What ran is read back and asserted."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from pauli_model import pauli_priors
from pauli_relay_model import PauliRelayModel
from test_gpu_pauli import frozen, tiles_of
from test_gpu_pauli_relay import device_entry, gammas_of, host_entry, same
from test_pauli_relay_cpu import KIB159, WIDTH_TABLE, lib_plan

pytestmark = pytest.mark.gpu
F = np.float32
LEGS, STOP_AFTER, BATCH = [3, 2, 2, 2], 2, 40


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


def padded(H, n, empty):
    """H with `empty` empty checks behind its rows and isolated qubits behind its columns up to n."""
    H = sp.csc_matrix(H)
    s, n0 = H.shape
    out = sp.csc_matrix((H.data, H.indices, np.concatenate([H.indptr, np.full(n - n0, H.indptr[-1], dtype=H.indptr.dtype)])),
                        shape=(s + empty, n))
    assert out.nnz == H.nnz and np.diff(out.indptr)[n0:].sum() == 0
    return out


@functools.lru_cache(maxsize=None)
def width_case(n):
    """-> (Hx, Hz, probs, gammas, sx, sz, model output).  The core's qubits have Pauli probabilities around 0.04 each, the
    isolated ones of 0.15 ... 0.32 (priors of both signs and of small magnitude); row b is sampled at 0.2 ... 2.2 times the
    core's probabilities.  Every empty check's entry is 0, but for the first empty Hz check in row 0 and the first empty Hx
    check in row 1: those rows can never converge."""
    ldpc = _ldpc()
    empty = WIDTH_TABLE[n][0]
    rep = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.uint8)
    cx, cz = ldpc.codes.hypergraph_product(rep, rep)
    cx, cz = sp.csc_matrix(cx), sp.csc_matrix(cz)
    assert cx.shape == cz.shape == (6, 13)
    Hx, Hz = padded(cx, n, empty // 2), padded(cz, n, empty // 2)
    rng = np.random.default_rng(n)
    probs = np.concatenate([0.04 * rng.uniform(0.5, 1.5, (13, 3)), rng.uniform(0.15, 0.32, (n - 13, 3))])
    scale = rng.permutation(np.linspace(0.2, 2.2, BATCH))
    edges = np.cumsum(probs[None, :13, :] * scale[:, None, None], axis=2)
    pauli = (rng.random((BATCH, 13, 1)) >= edges).sum(axis=2)                      # 0 = X, 1 = Y, 2 = Z, 3 = I
    ex, ez = (pauli <= 1).astype(np.uint8), ((pauli == 1) | (pauli == 2)).astype(np.uint8)
    sx, sz = np.zeros((BATCH, 6 + empty // 2), dtype=np.uint8), np.zeros((BATCH, 6 + empty // 2), dtype=np.uint8)
    sx[:, :6], sz[:, :6] = ldpc.codes.syndromes_of(cx, ez), ldpc.codes.syndromes_of(cz, ex)
    sz[0, 6], sx[1, 6] = 1, 1
    priors = pauli_priors(probs)
    assert (priors[:, 13:] < 0).any() and (priors[:, 13:] > 0).any()
    g = gammas_of(len(LEGS), n, seed=n)
    want = frozen_out(PauliRelayModel(Hx, Hz, priors, g, LEGS, stop_after=STOP_AFTER).decode(sx, sz))
    frozen(sx, sz)
    gx, gz, conv, its, sol, M = want
    # preconditions, on the model alone
    assert not conv[:2].any() and 0 < conv.sum() < BATCH, (n, int(conv.sum()))
    assert set(sol.tolist()) == {0, 1, 2} and len(set(its.tolist())) >= 4, (n, np.bincount(sol).tolist(), sorted(set(its.tolist())))
    assert (gx[:, 13:] | gz[:, 13:]).any() and not (gx[:, 13:] | gz[:, 13:]).all()      # isolated qubits that are no I, and some that are
    return Hx, Hz, probs, g, sx, sz, want


def frozen_out(want):
    frozen(*want)
    return want


def decoder(ldpc, case, variant=0):
    Hx, Hz, probs, g, _, _, _ = case
    return ldpc.PauliRelayMinSumDecoder(Hx, Hz, None, LEGS[0], pauli_probs=probs, legs=len(LEGS), leg_iters=LEGS[1], gammas=g,
                                        stop_after=STOP_AFTER, kernel_variant=variant)


@pytest.mark.parametrize("n", sorted(WIDTH_TABLE))
def test_every_width_of_the_table_equals_the_model(ldpc, gpu, n):
    """One row of the table, automatic selection: the tier and the width are asserted BEFORE the decode; the whole batch of
    40 through the device entry and the host entry, then a ragged prefix.  n = 6705 is the one-syndrome state of exactly
    159 KiB, the largest the planner admits on chip: with the kernel's static LDS it is 128 bytes short of a CU's 160 KiB."""
    empty, tier, S, _ = WIDTH_TABLE[n]
    case = width_case(n)
    Hx, Hz, probs, g, sx, sz, want = case
    s = Hx.shape[0] + Hz.shape[0]
    assert (s, Hx.shape[1]) == (12 + empty, n)
    plan = lib_plan(s, n, 48, 0)
    assert plan[:2] == (tier, S)
    if n == 6705:
        assert plan == (1, 1, KIB159) and lib_plan(s + 1, n, 48, 0)[:2] == (2, 64)
    dec = decoder(ldpc, case)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0), (dec.info(), tier, S)
    what = f"Pauli relay n {n} tier {tier} S {S}"
    same(device_entry(dec, sx, sz), want, f"{what}, batch {BATCH}")
    print(f"{what}: batch {BATCH}, tile_syndromes {dec.tile_syndromes}, last_grid {dec.last_grid}, converged {int(want[2].sum())}, "
          f"solutions {np.bincount(want[4]).tolist()}")
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, tiles_of(BATCH, S))
    same(host_entry(dec, sx, sz), want, f"{what}, host entry")
    same(device_entry(dec, sx[:23], sz[:23]), want, f"{what}, batch 23", slice(0, 23))
    assert dec.last_grid == tiles_of(23, S)
    dec.close()


@pytest.mark.parametrize("n", [32, 2560, 6705])
def test_the_on_chip_rows_in_the_unlimited_tier(ldpc, gpu, n):
    """The same inputs with the tier forced: S = 64 in a workspace slot, whatever the on-chip width was."""
    case = width_case(n)
    _, _, _, _, sx, sz, want = case
    dec = decoder(ldpc, case, variant=2)
    assert (dec.kernel, dec.tile_syndromes) == (2, 64)
    same(device_entry(dec, sx, sz), want, f"Pauli relay n {n} forced unlimited")
    assert dec.last_grid == 1
    dec.close()
