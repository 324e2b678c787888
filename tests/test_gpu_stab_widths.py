"""The stabilizer min-sum kernel (stab_kernels.hpp) at EVERY tile width, under both LDS budgets and in the unlimited tier by
size, against the numpy model of its rule (tests/stab_model.py): equality in every element -- gx, gz, flags, iteration
counts, and the three LLR planes as bit patterns; no tolerance.  The pattern of tests/test_gpu_pauli_relay_widths.py.

The kernel indexes every row of MX, MY, MZ, the records and the syndromes by `<< sh` with `l = t & (S - 1)`, `q = t >> sh`,
`Q = T >> sh`: at S = 64 a lane is shared by 8 threads of the on-chip kernel, at S = 1 by all 512, which then meet in
`sh_bad[0]`.  At S < 64 the lanes of one wave sit on different checks, so on edges of different types: the case the
conditional-move selects of `edge()` are there for.  tests/test_gpu_stab.py runs S = 64, 32 and 8 on chip only.

The graph is a small core with all three edge types -- the hypergraph product of two 3-bit repetition checks under the
single-qubit Cliffords of default_rng(0), n = 13, 12 checks, 19 X-, 9 Z- and 12 Y-type edges -- padded with isolated qubits
and empty checks until a lane has the size of a row of STAB_WIDTH_TABLE (tests/test_stab_cpu.py holds the table against the
planner).  The model loops over the edges in Python, so its cost stays that of the core.  An isolated qubit is no idle
ballast: its priors have both signs, and its decision enters gx, gz and the three LLR planes of every column.  Every case
asserts ON THE MODEL, before anything touches the GPU, that its batch holds converged and unconverged columns, at least three
iteration counts, and isolated qubits that are decided I and others that are not.  What ran is read back and asserted."""
import functools

import numpy as np
import pytest

from pauli_model import pauli_priors
from stab_model import StabMinSumModel, symplectic_syndromes
from test_gpu_pauli import frozen, same, tiles_of
from test_gpu_pauli_relay_widths import padded
from test_gpu_stab import device_entry, host_entry, mixed
from test_stab_cpu import KIB159, STAB_WIDTH_REC_WORDS, STAB_WIDTH_TABLE, stab_lib_plan, stab_width_core

pytestmark = pytest.mark.gpu
BATCH, MAX_ITERS = 40, 12


@functools.lru_cache(maxsize=None)
def width_case(n):
    """-> (Sx, Sz, probs, s, model output).  The core's qubits have Pauli probabilities around 0.04 each, the isolated ones of
    0.15 ... 0.32 (priors of both signs and of small magnitude); column b is sampled on the core at 0.2 ... 2.2 times its
    probabilities.  Every empty check's entry is 0, but for the first empty check in column 0: that column can never
    converge."""
    empty = STAB_WIDTH_TABLE[n][0]
    cx, cz = stab_width_core()
    Sx, Sz = padded(cx, n, empty), padded(cz, n, empty)
    rng = np.random.default_rng(n)
    probs = np.concatenate([0.04 * rng.uniform(0.5, 1.5, (13, 3)), rng.uniform(0.15, 0.32, (n - 13, 3))])
    scale = rng.permutation(np.linspace(0.2, 2.2, BATCH))
    edges = np.cumsum(probs[None, :13, :] * scale[:, None, None], axis=2)
    pauli = (rng.random((BATCH, 13, 1)) >= edges).sum(axis=2)                      # 0 = X, 1 = Y, 2 = Z, 3 = I
    ex, ez = (pauli <= 1).astype(np.uint8), ((pauli == 1) | (pauli == 2)).astype(np.uint8)
    s = np.zeros((BATCH, 12 + empty), dtype=np.uint8)
    s[:, :12] = symplectic_syndromes(cx, cz, ex, ez)
    s[0, 12] = 1
    priors = pauli_priors(probs)
    assert all((priors[k, 13:] < 0).any() and (priors[k, 13:] > 0).any() for k in range(3))
    want = StabMinSumModel(Sx, Sz, priors, MAX_ITERS).decode(s)
    frozen(s, *want)
    gx, gz, conv, its, G = want
    # preconditions, on the model alone
    assert not conv[0] and 0 < conv.sum() < BATCH, (n, int(conv.sum()))
    assert len(set(its.tolist())) >= 3, (n, sorted(set(its.tolist())))
    assert (gx[:, 13:] | gz[:, 13:]).any() and not (gx[:, 13:] | gz[:, 13:]).all()      # isolated qubits that are no I, and some that are
    return Sx, Sz, probs, s, want


def decoder(ldpc, case, variant=0):
    Sx, Sz, probs, _, _ = case
    return ldpc.StabilizerMinSumDecoder(Sx, Sz, None, MAX_ITERS, pauli_probs=probs, kernel_variant=variant)


@pytest.mark.parametrize("n", sorted(STAB_WIDTH_TABLE))
def test_every_width_of_the_table_equals_the_model(ldpc, gpu, n):
    """One row of the table, automatic selection: the tier and the width are asserted BEFORE the decode; the whole batch of
    40 through the device entry and the host entry, then a ragged prefix of 23.  n = 6725 is the window where the 159 KiB
    budget yields S = 2; n = 13550 is the one-syndrome state of exactly 159 KiB, the largest the planner admits on chip."""
    empty, _, tier, S, _ = STAB_WIDTH_TABLE[n]
    case = width_case(n)
    Sx, Sz, probs, s, want = case
    r = Sx.shape[0]
    assert Sx.shape == Sz.shape == (12 + empty, n)
    plan = stab_lib_plan(r, n, STAB_WIDTH_REC_WORDS, 0)
    assert plan[:2] == (tier, S)
    if n == 13550:
        assert plan == (1, 1, KIB159) and stab_lib_plan(r + 1, n, STAB_WIDTH_REC_WORDS, 0)[:2] == (2, 64)
    mixed(want[2], BATCH)
    dec = decoder(ldpc, case)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, 0), (dec.info(), tier, S)
    assert (dec.n, dec.rows) == (n, r)
    what = f"stabilizer min-sum n {n} tier {tier} S {S}"
    same(device_entry(dec, s), want, f"{what}, batch {BATCH}")
    print(f"{what}: batch {BATCH}, tile_syndromes {dec.tile_syndromes}, last_grid {dec.last_grid}, converged {int(want[2].sum())}, "
          f"iteration counts {sorted(set(want[3].tolist()))}")
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (tier, S, tiles_of(BATCH, S))
    same(host_entry(dec, s), want, f"{what}, host entry")
    assert dec.last_grid == tiles_of(BATCH, S)
    same(device_entry(dec, s[:23]), want, f"{what}, batch 23", slice(0, 23))
    assert dec.last_grid == tiles_of(23, S)
    dec.close()


@pytest.mark.parametrize("n", [80, 5120, 13550])
def test_the_on_chip_rows_in_the_unlimited_tier(ldpc, gpu, n):
    """The same inputs with the tier forced: S = 64 in a workspace slot, whatever the on-chip width was."""
    case = width_case(n)
    _, _, _, s, want = case
    mixed(want[2], BATCH)
    dec = decoder(ldpc, case, variant=2)
    assert (dec.kernel, dec.tile_syndromes, dec.last_grid) == (2, 64, 0)
    same(device_entry(dec, s), want, f"stabilizer min-sum n {n} forced unlimited")
    assert dec.last_grid == 1
    dec.close()
