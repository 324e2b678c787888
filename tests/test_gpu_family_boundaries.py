"""Pinned record forms of the joint X/Z (Pauli) decoder, the layered schedule and the entries with per-syndrome priors
against their numpy models (tests/pauli_model.py, layered_model.py, priors_model.py): equality in every element, the LLRs
as bit patterns, no tolerance.  Each case is built to reach one path of a kernel that the other suites do not reach, and
asserts ON THE MODEL or on the priors alone, before the GPU is touched, that its input really gets there.  All shapes have
n <= 400 and batch 65: one full tile and a ragged one at every S <= 64.

  1  Pauli record forms on BOTH sides (pauli_kernels.hpp: its own copies of the masks around `d0 == 32` and `deg == 64`, the
     `zrow` branch of `edge()`, the second pass of the per-edge record that re-runs `edge()` and restores `hard`): checks of
     degree 31, 32, 33, 63, 64 and 65 among the Hx rows and again among the Hz rows, the minimum at the last position
     alone and the top sign bit of a word set in some columns
  2  the same degrees under the layered schedule (layered_kernels.hpp: the write-back that keeps the OLD record in registers
     while it stores the new one, separately for the low and the high sign word) and under the floats and given entries of
     both schedules (minsum_kernels.hpp and layered_kernels.hpp with SRC != kMsPriorTable), which had seen no check of
     degree above 8
  3  a layered handle with no layer, K == 0 (layered_kernels.hpp: the extra barrier of the iteration loop)"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import priors_model as pm
from layered_model import LayeredMinSumModel
from minsum_model import llr_of_probs
from pauli_model import PauliMinSumModel, pauli_priors
from test_gpu_minsum import _device as ms_device
from test_gpu_minsum import _same as ms_same
from test_gpu_pauli import device_entry as pauli_device
from test_gpu_pauli import frozen
from test_gpu_pauli import same as pauli_same
from test_gpu_priors import _entry as priors_entry

pytestmark = pytest.mark.gpu
F = np.float32
B = 65
DEGREES = (31, 32, 33, 63, 64, 65)


def syndromes_of(Hd, e):
    return np.ascontiguousarray(((Hd.astype(np.int64) @ e.T.astype(np.int64)) % 2).T, dtype=np.uint8)


def first_sweep_preconditions(b, syn_col, what):
    """b: the first-sweep values b_k of one check, identical in every column (every message is +0); syn_col [B]: its syndrome
    entries.  The LAST position alone has the smallest |b| (so `a` is the last position and m2 comes from elsewhere), and
    the sign the sweep writes for the last position -- and for position 31, the top bit of the first sign word, where the
    check has one -- is set in some columns and not in all: sign_k = par ^ neg_k with par = syndrome ^ XOR neg."""
    deg = len(b)
    mag, neg = np.abs(b), b < 0
    assert int(np.argmin(mag)) == deg - 1 and (mag[:-1] > mag[-1]).all(), f"{what}: the minimum is not at the last position alone"
    assert neg[-1] and neg.sum() == (2 if deg > 32 else 1), what
    par = (syn_col != 0) ^ (neg.sum() % 2 == 1)
    sign = par[:, None] ^ neg[None, :]                                    # [column][position]
    assert sign[:, deg - 1].any() and not sign[:, deg - 1].all(), f"{what}: the top sign bit is set in no column / in every column"
    if deg >= 32:
        assert neg[31] and sign[:, 31].any() and not sign[:, 31].all(), what


# ---- 1. Pauli -------------------------------------------------------------------------------------------------------------
# check: (first qubit, degree) on consecutive qubits; the Hz checks take the degrees in the reverse order, 6 qubits further on,
# so that no wide check of one side has the support or the last qubit of one of the other side
HX_WIDE = {2: (0, 31), 3: (31, 32), 4: (63, 33), 5: (96, 63), 6: (159, 64), 7: (223, 65)}
HZ_WIDE = {2: (6, 65), 3: (71, 64), 4: (135, 63), 5: (198, 33), 6: (231, 32), 7: (263, 31)}
PAULI_N = 300


@functools.lru_cache(maxsize=None)
def pauli_edges():
    """Hx and Hz, 30 checks x 300 qubits each: check 0 empty, check 1 of degree 1 (qubit 296 / 297), checks 2 ... 7 the wide
    ones on the qubits 0 ... 293, 22 random checks of degree 3 ... 6 over the qubits 0 ... 297; qubit 298 sits in one random
    Hx check only, qubit 299 in no check (Y likelier than I).  Per-qubit probabilities made from wanted prior tables: every
    prior in (0.9, 4) except, per wide Hx check i, prior_z of its last qubit = -0.04 i and of its qubit at position 31
    (degree > 32) = -0.5, and the same in prior_x for the wide Hz checks.  65 syndrome pairs: 40 of sampled errors, 25 arbitrary."""
    rng = np.random.default_rng(47)
    r, n = 30, PAULI_N
    sides = []
    for wide, lone in ((HX_WIDE, 296), (HZ_WIDE, 297)):
        Hd = np.zeros((r, n), dtype=np.uint8)
        Hd[1, lone] = 1
        for i, (first, deg) in wide.items():
            Hd[i, first:first + deg] = 1
        for i in range(8, r):
            Hd[i, rng.choice(298, size=int(rng.integers(3, 7)), replace=False)] = 1
        assert Hd[0].sum() == 0 and Hd[1].sum() == 1 and sorted(int(Hd[i].sum()) for i in wide) == list(DEGREES) and Hd[8:].sum(axis=1).max() <= 6
        sides.append(Hd)
    Hx, Hz = sides
    Hx[8, 298] = 1
    assert Hx[:, 298].sum() == 1 and Hz[:, 298].sum() == 0 and Hx[:, 299].sum() == Hz[:, 299].sum() == 0
    llr = rng.uniform(0.9, 4.0, size=(3, n))                               # wanted prior_x, prior_y, prior_z
    for wide, table in ((HX_WIDE, 2), (HZ_WIDE, 0)):                       # an Hx check reads min(GY, GZ), an Hz check min(GY, GX)
        for i, (first, deg) in wide.items():
            llr[table, first + deg - 1] = -0.04 * i
            if deg > 32:
                llr[table, first + 31] = -0.5
    llr[:, 299] = [2.0, -0.7, 1.5]
    rest = 1.0 / (1.0 + np.exp(-llr).sum(axis=0))
    probs = np.ascontiguousarray((rest[None, :] * np.exp(-llr)).T)         # [n][3]
    e = [(rng.random((B, n)) < 0.02).astype(np.uint8) for _ in range(2)]
    sx, sz = syndromes_of(Hx, e[1]), syndromes_of(Hz, e[0])
    sx[40:], sz[40:] = rng.integers(0, 2, size=(25, r)), rng.integers(0, 2, size=(25, r))
    frozen(Hx, Hz, probs, sx, sz)
    return Hx, Hz, probs, sx, sz


def pauli_first_sweep(priors, Hd, zrow, clip):
    """b_k of every check of one side in sweep 1, from the prior tables alone: TX = TZ = +0 and every message +0, so
    GW = prior_W and b_k = clamp((u_k - 0) - w_k) with u = min(GY, own), w = other < 0 ? other : +0 (the header's rule)."""
    px, py, pz = priors
    own, other = (px, pz) if zrow else (pz, px)
    u = np.where(py < own, py, own)
    w = np.where(other < 0, other, F(0.0))
    b = np.minimum(np.maximum((u - F(0.0)) - w, -F(clip)), F(clip)).astype(F)
    return [b[np.nonzero(row)[0]] for row in Hd]


def pauli_edges_reach_their_paths():
    """The preconditions of the fixture, from the priors alone."""
    Hx, Hz, probs, sx, sz = pauli_edges()
    priors = pauli_priors(probs)
    assert (priors[2] < 0).sum() == 6 + 4 and (priors[0] < 0).sum() == 6 + 4 and (priors[1] < 0).sum() == 1
    for name, Hd, wide, syn, zrow in (("Hx", Hx, HX_WIDE, sx, False), ("Hz", Hz, HZ_WIDE, sz, True)):
        b = pauli_first_sweep(priors, Hd, zrow, 1e6)
        for i, (first, deg) in wide.items():
            assert len(b[i]) == deg
            first_sweep_preconditions(b[i], syn[:, i], f"{name} check {i} of degree {deg}")


@functools.lru_cache(maxsize=None)
def pauli_edges_want(alpha, clip):
    Hx, Hz, probs, sx, sz = pauli_edges()
    want = PauliMinSumModel(Hx, Hz, pauli_priors(probs), 25, alpha=alpha, clip=clip).decode(sx, sz)
    frozen(*want)
    return want


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_pauli_record_forms_at_degrees_31_to_65_on_both_sides(ldpc, gpu, alpha, variant):
    """pauli_kernels.hpp, the records of Hx rows (zrow false) and of Hz rows (zrow true): four words with the mask
    `(1u << d0) - 1u` at degree 31 and `d0 == 32` at 32; five words with `(1u << (deg - 32)) - 1u` at 33 and 63 and
    `deg == 64` at 64; a word per edge with the second `edge()` pass at 65."""
    Hx, Hz, probs, sx, sz = pauli_edges()
    pauli_edges_reach_their_paths()
    want = pauli_edges_want(alpha, 1e6)
    gx, gz, conv, its, G = want
    assert 0 < conv.sum() < B and len(set(its.tolist())) >= 3, (int(conv.sum()), sorted(set(its.tolist())))
    assert (gx[:, 299] & gz[:, 299]).all()                                 # the qubit in no check is a Y in every column
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, 25, alpha=alpha, pauli_probs=probs, kernel_variant=variant, check=False)
    assert dec.kernel == variant and dec.tile_syndromes <= 64 and (dec.n, dec.rows_x, dec.rows_z) == (PAULI_N, 30, 30)
    pauli_same(pauli_device(dec, sx, sz), want, f"alpha {alpha}, tier {variant}")
    assert dec.last_grid == -(-B // dec.tile_syndromes) >= 2
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_pauli_record_forms_with_every_value_clamped(ldpc, gpu, variant):
    """clip below the smallest |prior|: `ms_clamp` engages on every edge of both sides, every |b| is clip, so `mag < m1` is
    never true, `a` stays kMsNone and every record holds alpha * clip twice; what is left to differ is the signs."""
    Hx, Hz, probs, sx, sz = pauli_edges()
    priors = pauli_priors(probs)
    clip = float(F(0.5) * np.abs(priors).min())
    assert 0 < clip < np.abs(priors).min()
    for Hd, zrow in ((Hx, False), (Hz, True)):
        assert all((np.abs(b) == F(clip)).all() for b in pauli_first_sweep(priors, Hd, zrow, clip))
    want, loose = pauli_edges_want(1.0, clip), pauli_edges_want(1.0, 1e6)
    assert (want[4].view(np.int32) != loose[4].view(np.int32)).any(axis=(1, 2)).all()
    dec = ldpc.PauliMinSumDecoder(Hx, Hz, None, 25, alpha=1.0, clip=clip, pauli_probs=probs, kernel_variant=variant, check=False)
    assert dec.kernel == variant
    pauli_same(pauli_device(dec, sx, sz), want, f"clip {clip}, tier {variant}")
    dec.close()


# ---- 2. layered and per-syndrome priors --------------------------------------------------------------------------------------
WIDE = {2: (0, 31), 3: (31, 32), 4: (63, 33), 5: (96, 63), 6: (159, 64), 7: (223, 65)}    # check: (first bit, degree)


@functools.lru_cache(maxsize=None)
def family_edges():
    """tests/test_gpu_model_boundaries.py's record_edges with a check of degree 33 and one of degree 64 added: 32 checks x
    300 bits, check 0 empty, check 1 of degree 1, checks 2 ... 7 of degree 31 / 32 / 33 / 63 / 64 / 65 on the consecutive bits
    0 ... 287, 24 random checks of degree 3 ... 6 over the bits 0 ... 297; bit 298 sits in check 8 only, bit 299 in none
    (negative prior).  In each wide check the LAST bit has the smallest |prior| and a negative prior, and where the check has
    one, so has its bit at position 31 (with a larger |prior|).  65 syndromes: 40 of sampled errors, 25 arbitrary."""
    rng = np.random.default_rng(33)
    s, n = 32, 300
    Hd = np.zeros((s, n), dtype=np.uint8)
    Hd[1, 293] = 1
    for i, (first, deg) in WIDE.items():
        Hd[i, first:first + deg] = 1
    for i in range(8, s):
        Hd[i, rng.choice(298, size=int(rng.integers(3, 7)), replace=False)] = 1
    Hd[8, 298] = 1
    assert Hd[0].sum() == 0 and Hd[1].sum() == 1 and Hd[:, 298].sum() == 1 and Hd[:, 299].sum() == 0
    assert [int(Hd[i].sum()) for i in WIDE] == list(DEGREES) and Hd[8:].sum(axis=1).max() <= 7
    prior = llr_of_probs(rng.uniform(0.01, 0.3, n))
    assert prior.min() > 0.8
    prior[299] = F(-0.8)
    prior[295] = F(1e-40)          # a subnormal prior (bits 288 ... 297 sit in random checks only)
    prior[296] = F(-0.0)
    for i, (first, deg) in WIDE.items():
        prior[first + deg - 1] = F(-0.05 * i)
        if deg > 32:
            prior[first + 31] = F(-0.5)
    e = (rng.random((B, n)) < 0.03).astype(np.uint8)
    syn = syndromes_of(Hd, e)
    syn[40:, :] = rng.integers(0, 2, size=(25, s))
    # per-row priors: the base prior scaled per row by a positive factor (an exact power of two or not: both kinds)
    factor = np.concatenate([[0.5, 1.0, 2.0], rng.uniform(0.5, 2.0, B - 3)]).astype(F)
    pri = (prior[None, :] * factor[:, None]).astype(F)
    # two tables for the given entry: any mix of them keeps the property (the last bits shrink, the others grow)
    special = np.zeros(n, dtype=bool)
    special[[first + deg - 1 for first, deg in WIDE.values()]] = True
    t1 = np.where(special, prior * F(0.5), prior * F(1.25)).astype(F)
    given = rng.integers(0, 256, size=(B, n), dtype=np.uint8)
    frozen(Hd, prior, syn, pri, t1, given)
    return sp.csc_matrix(Hd), Hd, prior, syn, pri, t1, given


def family_preconditions(rows, syn, what):
    """rows [B][n] (or one row [n]): in sweep 1 every message is +0, so b_k is the prior itself (|prior| < clip)."""
    rows = np.atleast_2d(rows)
    for i, (first, deg) in WIDE.items():
        b = rows[:, first:first + deg]
        mag, neg = np.abs(b), b < 0
        assert (np.argmin(mag, axis=1) == deg - 1).all() and (mag[:, :-1] > mag[:, -1:]).all(), f"{what}, check {i}: the minimum is not at the last position alone"
        assert neg[:, -1].all() and (neg.sum(axis=1) == (2 if deg > 32 else 1)).all(), (what, i)
        first_sweep_preconditions(b[0], syn[:, i], f"{what}, check {i}")     # (the signs of a row are those of row 0)
        assert (neg == neg[0]).all()


def family_edges_reach_their_paths():
    """On the priors alone: the base prior, every per-row prior, both tables and every row of their mix by the given bytes."""
    H, Hd, prior, syn, pri, t1, given = family_edges()
    family_preconditions(prior, syn, "base prior")
    family_preconditions(pri, syn, "per-row priors")
    family_preconditions(t1, syn, "second table")
    family_preconditions(pm.select_priors(given, prior, t1), syn, "selected priors")
    assert len(set(map(bytes, pri))) == B and (given > 1).any() and (pm.select_priors(given, prior, t1) != prior[None, :]).any()


@functools.lru_cache(maxsize=None)
def family_want(kind, schedule):
    H, Hd, prior, syn, pri, t1, given = family_edges()
    if kind == "plain":
        model = LayeredMinSumModel(H, prior, 20)
        want = model.decode(syn)
        layers = model.layers
    else:
        want = pm.model_of(schedule, H, 20).decode(syn, pri if kind == "floats" else pm.select_priors(given, prior, t1))
        layers = None
    frozen(*want)
    assert want[1].any() and not want[1].all(), f"{kind} {schedule}: the model converges on every column or on none"
    assert want[0][:, 299].all()
    return want, layers


@pytest.mark.parametrize("variant", [1, 2])
def test_layered_record_forms_at_degrees_31_to_65(ldpc, gpu, variant):
    """layered_kernels.hpp, the write-back of a check's record while the old one is still needed: degrees 31 and 32 (one sign
    word, masks at d0 == 32), 33, 63 and 64 (the high sign word kept and stored separately, mask at deg == 64), 65 (a word
    per edge).  The six wide checks share no bit, so first fit puts them into one layer: they run side by side."""
    H, Hd, prior, syn, _, _, _ = family_edges()
    family_edges_reach_their_paths()
    want, layers = family_want("plain", "layered")
    assert len(layers) == 5 and set(WIDE) <= set(layers[0]) and len(layers[0]) > len(WIDE), [len(ly) for ly in layers]
    dec = ldpc.MinSumDecoder(H, None, 20, channel_llr=prior, kernel_variant=variant, schedule="layered")
    assert dec.kernel == variant and dec.layers == len(layers) and dec.info().tile_syndromes <= 64
    ms_same(ms_device(dec, np.array(syn)), want, f"layered, tier {variant}")
    assert dec.info().last_grid == -(-B // dec.info().tile_syndromes) >= 2
    dec.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_priors_entries_on_the_record_forms(ldpc, gpu, schedule, variant):
    """minsum_kernels.hpp (flooding) and layered_kernels.hpp (layered) with SRC != kMsPriorTable on checks of degree 31, 32,
    33, 63, 64 and 65: the floats entry with a prior row per syndrome (the base prior times a positive factor), then the
    given entry with two tables that both keep the minimum at the last position."""
    H, Hd, prior, syn, pri, t1, given = family_edges()
    family_edges_reach_their_paths()
    dec = ldpc.MinSumDecoder(H, 0.05, 20, kernel_variant=variant, schedule=schedule)
    info = dec.info()
    assert (info.kernel, info.priors_kernel) == (variant, variant) and info.priors_tile_syndromes <= 64
    grid = -(-B // info.priors_tile_syndromes)
    ms_same(priors_entry(dec, syn, pri, "priors"), family_want("floats", schedule)[0], f"{schedule} tier {variant}, floats")
    assert dec.info().last_grid == grid >= 2
    dec.set_conditional_priors(prior, t1)
    ms_same(priors_entry(dec, syn, given, "given"), family_want("given", schedule)[0], f"{schedule} tier {variant}, given")
    assert dec.info().last_grid == grid
    dec.close()


# ---- 3. layered with no layer ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
def test_layered_with_no_edge_and_no_layer(ldpc, gpu, variant):
    """layered_kernels.hpp with K == 0: the loop over the layers has no barrier of its own, so the iteration loop takes the
    extra one.  3 checks, 5 bits, no edge: an all-zero syndrome row converges at iteration 1 with err = (prior <= 0), a row
    with a set entry is matched by no error and runs all 3 iterations; L stays the prior in both."""
    H = sp.csc_matrix((3, 5), dtype=np.uint8)
    prior = np.array([1.5, -0.25, 0.0, -0.0, 3.0], dtype=F)
    syn = np.zeros((B, 3), dtype=np.uint8)
    syn[1::3, 0], syn[2::3, 2], syn[5::6, 1] = 1, 7, 1
    zero = ~syn.any(axis=1)
    assert zero.sum() == 22 and zero[0] and not zero[B - 1]
    model = LayeredMinSumModel(H, prior, 3)
    want = model.decode(syn)
    assert model.K == 0 and np.array_equal(want[1], zero) and np.array_equal(want[2], np.where(zero, 1, 3))
    assert (want[0] == (prior <= 0)[None, :]).all() and (want[3].view(np.int32) == prior.view(np.int32)[None, :]).all()
    dec = ldpc.MinSumDecoder(H, None, 3, channel_llr=prior, kernel_variant=variant, schedule="layered")
    assert dec.kernel == variant and dec.layers == 0
    ms_same(ms_device(dec, syn), want, f"no layer, tier {variant}")
    ms_same(dec.decode_batch_host(syn, want_llr=True), want, f"no layer, tier {variant}, host entry")
    dec.close()
