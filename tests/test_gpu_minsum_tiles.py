"""Min-sum and relay decoders on the GPU at EVERY tile width and with SLOT REUSE, against the numpy models of their rules
(tests/minsum_model.py, tests/relay_model.py): equality in every element -- errors, flags, iteration counts, solution
counts, and the LLRs as bit patterns; the arithmetic has no division and no transcendental, so there is no tolerance.

What ran is read back and asserted (`info().kernel`, `.tile_syndromes`, `.last_grid`), so a case that misses its width or
whose workgroups never take a second tile fails instead of passing on another path:

  a. every row of the tile-plan table (tests/test_tile_plan_cpu.py): S = 64 ... 1 on chip under both LDS budgets and the
     step to the unlimited tier by size, with per-bit priors and a waterfall across the batch;
  b. a second tile in the same LDS block / workspace slot, forced: the grid capped at 1 and 3 workgroups
     (LDPC_MS_GRID_MAX, experiments build), one handle used for 1, 7 and 2 tiles in a row;
  c. the same in the product build with no knob: more tiles than the device hosts workgroups;
  d. two handles of different widths alive together (the dynamic-LDS limit belongs to the kernel, not to a handle).

Model cost.  The models loop over the edges in Python: their time is proportional to n x iterations and nearly
independent of the batch.  Measured on one CPU core each, two models running side by side: min-sum n = 13824, 5 iterations, 165
columns 6.9 s (n = 12288, 6 iterations: 5.2 s; n = 6144, 8 iterations: 3.8 s); relay n = 13824, legs [2, 1, 1]: 9.0 s
(n = 12288: 7.8 s; n = 6144, legs [3, 2, 2]: 3.3 s); every other shape below 3 s.  The iteration counts of SHAPES are
chosen so that no test spends more than about 10 s in a model; each result is computed once and shared."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from minsum_model import MinSumModel, llr_of_probs
from relay_model import RelayModel

pytestmark = pytest.mark.gpu

# ---- a. the table: (3,6)-regular n -> (tier, S) by size, and what makes the batch a waterfall ------------------------
# min-sum: n -> (tier, S, max_iters, rate); relay: n -> (tier, S, leg_iters, rate).  `rate`: the mean of the per-bit error
# probabilities (each bit's is rate x uniform(0.5, 1.5), its prior); row b of the batch is sampled at 0.1 ... 1.9 times
# them, so the rows run from nearly clean to hopeless.  Picked with the models on the CPU so that every batch has
# converged and unconverged rows and at least three iteration counts (asserted below on the model's output).
MS_SHAPES = {
    96: (1, 64, 10, 0.05),
    192: (1, 32, 10, 0.05),
    384: (1, 16, 10, 0.05),
    768: (1, 8, 10, 0.05),
    1536: (1, 4, 10, 0.05),
    3072: (1, 2, 10, 0.05),
    6144: (1, 1, 8, 0.05),       # inside the 79 KiB budget
    12288: (1, 1, 6, 0.05),      # inside the 159 KiB budget: one workgroup a CU
    13824: (2, 64, 5, 0.05),     # too large for LDS: the unlimited tier by size
}
RELAY_SHAPES = {
    96: (1, 32, [5, 3, 3], 0.05),
    192: (1, 16, [5, 3, 3], 0.05),
    384: (1, 8, [5, 3, 3], 0.05),
    768: (1, 4, [5, 3, 3], 0.05),
    1536: (1, 2, [5, 3, 3], 0.05),
    3072: (1, 1, [4, 2, 2], 0.05),
    6144: (1, 1, [3, 2, 2], 0.02),   # inside the 159 KiB budget
    12288: (2, 64, [2, 1, 1], 0.01),
    13824: (2, 64, [2, 1, 1], 0.01),
}
STOP_AFTER = 2


def _ldpc():
    import ldpcdecoders_jl_amd as m

    return m


def batch_of(S):
    """Two full tiles and more: 2 S + max(1, S / 2 + 5), at least 3."""
    return max(3, 2 * S + max(1, S // 2 + 5))


def ragged_prefix_of(S):
    """... and the prefix of it that is two full tiles and a ragged one for every S > 1, three tiles of one at S = 1."""
    return max(3, 2 * S + max(1, S // 2 - 5))


def gammas_of(legs, n, seed):
    """Leg 0 at 0.125, the others uniform in (-0.24, 0.66): both signs."""
    g = np.empty((legs, n), dtype=np.float32)
    g[0] = 0.125
    g[1:] = np.random.default_rng(seed).uniform(-0.24, 0.66, size=(legs - 1, n)).astype(np.float32)
    assert legs == 1 or ((g < 0).any() and (g > 0).any())
    return g


def waterfall_inputs(n, B, rate):
    """(H, prior f32 [n], syndromes [B][s]): per-bit priors, rows sampled at 0.1 ... 1.9 times the bits' probabilities."""
    ldpc = _ldpc()
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    rng = np.random.default_rng(n)
    probs = rate * rng.uniform(0.5, 1.5, n)
    scale = rng.permutation(np.linspace(0.1, 1.9, B))
    e = (rng.random((B, n)) < probs[None, :] * scale[:, None]).astype(np.uint8)
    prior = llr_of_probs(probs)
    assert len(set(prior.tolist())) > n // 2            # lanes and nodes are distinguishable
    return H, prior, ldpc.codes.syndromes_of(H, e)


@functools.lru_cache(maxsize=None)
def width_case(relay, n, S):
    """The inputs of a table row at tile width S and the model's output on them (computed once, never written to)."""
    B = batch_of(S)
    if relay:
        _, _, legs, rate = RELAY_SHAPES[n]
        H, prior, syn = waterfall_inputs(n, B, rate)
        g = gammas_of(len(legs), n, n + 1)
        want = RelayModel(H, prior, g, legs, stop_after=STOP_AFTER).decode(syn)
        conv, its = want[1], want[2]
    else:
        _, _, iters, rate = MS_SHAPES[n]
        H, prior, syn = waterfall_inputs(n, B, rate)
        g, legs = None, [iters]
        want = MinSumModel(H, prior, iters).decode(syn)
        conv, its = want[1], want[2]
    for x in want:
        x.setflags(write=False)
    # preconditions, on the model alone
    assert 0 < conv.sum() < B, (n, int(conv.sum()), B)
    if B >= 5:
        assert len(set(its.tolist())) >= 3, (n, sorted(set(its.tolist())))
    if relay:     # lanes in different legs: within one tile where a tile has more than one lane
        first = its <= legs[0]
        assert first.any() and (~first).any()
        if S > 1:
            assert any(first[k:k + S].any() and (~first[k:k + S]).any() for k in range(0, B, S)), n
    return H, prior, syn, g, legs, want


# ---- device and host entries, comparison ------------------------------------------------------------------------------

def make_decoder(ldpc, relay, H, prior, g, legs, variant=0, stop_after=STOP_AFTER):
    if relay:
        assert len(set(legs[1:])) <= 1          # the constructor takes one count for every leg after the first
        return ldpc.RelayMinSumDecoder(H, None, int(legs[0]), channel_llr=prior, legs=len(legs),
                                       leg_iters=int(legs[1]) if len(legs) > 1 else 0, gammas=g, stop_after=stop_after,
                                       kernel_variant=variant)
    return ldpc.MinSumDecoder(H, None, int(legs[0]), channel_llr=prior, kernel_variant=variant)


def device_entry(dec, relay, syn):
    """-> (err, conv, iters, solutions | None, llr f64), every output buffer pre-filled with a value no decode writes."""
    import torch

    B = syn.shape[0]
    d_syn = torch.from_numpy(np.ascontiguousarray(syn, dtype=np.uint8)).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, dec.n), 7.0, dtype=torch.float64, device="cuda")
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    sol = torch.full((B,), -7, dtype=torch.int32, device="cuda") if relay else None
    if relay:
        dec.decode_batch_device(d_syn, err, conv, llr, its, sol)
    else:
        dec.decode_batch_device(d_syn, err, conv, llr, its)
    torch.cuda.synchronize()
    return err.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy(), sol.cpu().numpy() if relay else None, llr.cpu().numpy()


def host_entry(dec, relay, syn):
    if relay:
        err, conv, llr, its, sol = dec.decode_batch_host(syn, want_llr=True, want_solutions=True)
        return err, conv, its, sol, llr
    err, conv, llr, its = dec.decode_batch_host(syn, want_llr=True)
    return err, conv, its, None, llr


def rows_of(want, relay, idx):
    """The model's output (min-sum: err, conv, iters, L; relay: err, conv, iters, solutions, M) at rows idx, as
    (err, conv, iters, solutions | None, LLR f32)."""
    if relay:
        return want[0][idx], want[1][idx], want[2][idx], want[3][idx], want[4][idx]
    return want[0][idx], want[1][idx], want[2][idx], None, want[3][idx]


def same(got, want, what):
    err, conv, its, sol, llr = got
    merr, mconv, mits, msol, mL = want
    assert err.shape == merr.shape and np.array_equal(err, merr), f"{what}: errors differ in {int((err != merr).any(axis=1).sum())} of {len(err)} columns"
    assert np.array_equal(conv, mconv), f"{what}: converged flags differ in columns {np.nonzero(conv != mconv)[0][:8].tolist()}"
    assert its.dtype == np.int32 and np.array_equal(its, mits), f"{what}: iteration counts differ in columns {np.nonzero(its != mits)[0][:8].tolist()}"
    if msol is not None:
        assert sol.dtype == np.int32 and np.array_equal(sol, msol), f"{what}: solution counts differ in columns {np.nonzero(sol != msol)[0][:8].tolist()}"
    assert llr.dtype == np.float64
    assert np.array_equal(llr.view(np.int64), mL.astype(np.float64).view(np.int64)), f"{what}: LLR bit patterns differ"


def tiles_of(B, S):
    return (B + S - 1) // S


# ---- a. every width ---------------------------------------------------------------------------------------------------

TABLE_CASES = [(False, n) for n in MS_SHAPES] + [(True, n) for n in RELAY_SHAPES]


@pytest.mark.parametrize("relay,n", TABLE_CASES, ids=[f"{'relay' if r else 'minsum'}-n{n}" for r, n in TABLE_CASES])
def test_every_width_of_the_table_equals_the_model(ldpc, gpu, relay, n):
    """One row of the table, automatic selection: the tier and the width are asserted BEFORE the decode; the whole batch
    (2 S + S / 2 + 5 syndromes) and its prefix of two full tiles and a ragged one go through the device entry, the rows of
    the widest and the narrowest width also through the host entry."""
    tier, S = (RELAY_SHAPES if relay else MS_SHAPES)[n][:2]
    H, prior, syn, g, legs, want = width_case(relay, n, S)
    B = syn.shape[0]
    dec = make_decoder(ldpc, relay, H, prior, g, legs)
    info = dec.info()
    assert (info.kernel, info.tile_syndromes, info.last_grid) == (tier, S, 0), (info, tier, S)
    what = f"{'relay' if relay else 'min-sum'} n {n} tier {tier} S {S}"
    same(device_entry(dec, relay, syn), rows_of(want, relay, slice(0, B)), f"{what}, batch {B}")
    info = dec.info()
    print(f"{what}: batch {B}, tile_syndromes {info.tile_syndromes}, last_grid {info.last_grid}")
    assert info.tile_syndromes == S and info.last_grid == tiles_of(B, S) >= 3
    Bp = ragged_prefix_of(S)
    assert Bp <= B and tiles_of(Bp, S) == 3 and (S == 1 or Bp % S != 0)
    same(device_entry(dec, relay, syn[:Bp]), rows_of(want, relay, slice(0, Bp)), f"{what}, batch {Bp}")
    assert dec.info().last_grid == 3
    if n in (96, 6144):
        same(host_entry(dec, relay, syn), rows_of(want, relay, slice(0, B)), f"{what}, host entry")
    dec.close()


@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
def test_the_unlimited_tier_forced_at_n_768(ldpc, gpu, relay):
    """kernel_variant = 2 at a size between BB-72 and "too large for LDS": 165 syndromes, two tiles of 64 and one of 37."""
    H, prior, syn, g, legs, want = width_case(relay, 768, 64)
    dec = make_decoder(ldpc, relay, H, prior, g, legs, variant=2)
    assert (dec.info().kernel, dec.info().tile_syndromes) == (2, 64)
    same(device_entry(dec, relay, syn), rows_of(want, relay, slice(0, 165)), "n 768 forced tier 2")
    assert dec.info().last_grid == 3
    dec.close()


# ---- b. a second tile in the same slot, forced ------------------------------------------------------------------------

NINE_LEGS = [30] + [20] * 8
SHORT_LEGS = [4, 3, 3]


def reuse_preconditions(conv, sol, B, S, strides):
    """With a grid of g workgroups tile k + g follows tile k in the same state.  For every stride: a lane converged in a tile
    and unconverged in the one that follows it in its slot, a lane for which the reverse holds, for relay a lane with
    solutions > 0 followed by solutions == 0 (where a stale `best` would show), and a ragged last tile behind a full one."""
    T = tiles_of(B, S)
    c = np.zeros(T * S, dtype=np.int64) - 1
    c[:B] = conv
    c = c.reshape(T, S)
    assert B % S != 0
    for g in strides:
        assert T > g, (T, g)
        a, b = c[:-g], c[g:]
        assert ((a == 1) & (b == 0)).any(), f"stride {g}: no lane converged, then unconverged"
        assert ((a == 0) & (b == 1)).any(), f"stride {g}: no lane unconverged, then converged"
        if sol is not None:
            f = np.zeros(T * S, dtype=np.int64) - 1
            f[:B] = sol
            f = f.reshape(T, S)
            assert ((f[:-g] > 0) & (f[g:] == 0)).any(), f"stride {g}: no lane with a solution, then without"


@functools.lru_cache(maxsize=None)
def bb72_reuse_case(kind):
    """BB-72 H_X, uniform prior 0.06, the 400 syndromes of errors at 0.06 (seed 3) of tests/test_gpu_relay.py in their
    order (the preconditions below hold for it as it is).  kind "minsum": 30 iterations.  "relay9": the nine legs
    [30, 20, ..., 20] of that file with stop_after = 3 -- the relay then converges all 400 (three solutions each), so no
    order of them has an unconverged lane behind a converged one; "relay3" therefore runs the same syndromes with the
    short legs [4, 3, 3] and stop_after = 2 of that file, which leave 120 of them without a solution, and carries the
    preconditions.  -> (H, prior, syn, gammas, legs, stop_after, model output)."""
    ldpc = _ldpc()
    Hx, _ = ldpc.codes.bivariate_bicycle_72_12_6()
    H = sp.csc_matrix(np.asarray(Hx, dtype=np.uint8))
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(72, 400, 0.06, seed=3))
    prior = llr_of_probs(np.full(72, 0.06))
    if kind == "minsum":
        g, legs, stop_after = None, [30], 1
        want = MinSumModel(H, prior, 30).decode(syn)
    else:
        legs, stop_after = (NINE_LEGS, 3) if kind == "relay9" else (SHORT_LEGS, 2)
        g = gammas_of(9, 72, 5)[:len(legs)]
        want = RelayModel(H, prior, g, legs, stop_after=stop_after).decode(syn)
        assert (want[2] <= legs[0]).any() and (want[2] > legs[0]).any()      # lanes in different legs
    for x in want:
        x.setflags(write=False)
    if kind == "relay9":
        assert want[1].all() and (want[3] == 3).all()
    else:
        reuse_preconditions(want[1], want[3] if kind != "minsum" else None, 400, 64, (1, 3))
    return H, prior, syn, g, legs, stop_after, want


@functools.lru_cache(maxsize=None)
def c240_reuse_case(relay):
    """The (240, 8, 4) code with per-bit priors of tests/test_gpu_minsum.py / test_gpu_relay.py, batch 130: nine tiles of 16
    on chip, three of 64 in the unlimited tier."""
    ldpc = _ldpc()
    H = sp.csc_matrix(ldpc.parity_check_matrix(240, 8, 4))
    rng = np.random.default_rng(11)
    probs = rng.uniform(1e-4, 0.45, 240)
    probs[[3, 77, 200]] = [0.6, 0.75, 0.9]
    e = (rng.random((130, 240)) < np.minimum(probs, 0.04)[None, :]).astype(np.uint8)
    syn = ldpc.codes.syndromes_of(H, e)
    prior = llr_of_probs(probs)
    if relay:
        g, legs = gammas_of(3, 240, 2), [8, 6, 6]
        want = RelayModel(H, prior, g, legs, stop_after=2).decode(syn)
    else:
        g, legs = None, [20]
        want = MinSumModel(H, prior, 20).decode(syn)
    for x in want:
        x.setflags(write=False)
    reuse_preconditions(want[1], want[3] if relay else None, 130, 16, (1, 3))
    reuse_preconditions(want[1], want[3] if relay else None, 130, 64, (1,))
    return H, prior, syn, g, legs, 2, want


def capped_decoder(ldpc, monkeypatch, cap, relay, case, variant):
    """The knob is read when the decoder is created; setting it selects the experiments build."""
    monkeypatch.setenv("LDPC_MS_GRID_MAX", str(cap))
    H, prior, _, g, legs, stop_after, _ = case
    dec = make_decoder(ldpc, relay, H, prior, g, legs, variant=variant, stop_after=stop_after)
    assert dec._L is ldpc._capi.lib(True)
    return dec


REUSE_CASES = [(kind, variant, cap) for kind in ("minsum", "relay9", "relay3") for variant in (1, 2) for cap in (1, 3)]


@pytest.mark.parametrize("kind,variant,cap", REUSE_CASES, ids=[f"{k}-tier{v}-grid{c}" for k, v, c in REUSE_CASES])
def test_bb72_tile_after_tile_in_one_slot_under_a_capped_grid(ldpc, gpu, monkeypatch, kind, variant, cap):
    """One handle, three calls in a row: 1 tile, then all 7 (the last one ragged) on `cap` workgroups, then 2 tiles of
    other syndromes -- every state a tile finds is what the tile or the call before left there."""
    relay = kind != "minsum"
    case = bb72_reuse_case(kind)
    syn, want = case[2], case[6]
    dec = capped_decoder(ldpc, monkeypatch, cap, relay, case, variant)
    assert (dec.info().kernel, dec.info().tile_syndromes, dec.info().last_grid) == (variant, 64, 0)
    what = f"{kind} BB-72 tier {variant} grid {cap}"
    for lo, hi in ((336, 400), (0, 400), (250, 350)):
        same(device_entry(dec, relay, syn[lo:hi]), rows_of(want, relay, slice(lo, hi)), f"{what}, columns {lo}:{hi}")
        tiles = tiles_of(hi - lo, 64)
        assert dec.info().last_grid == min(cap, tiles), (dec.info(), tiles)
        if hi - lo == 400:
            assert dec.info().last_grid == cap < tiles == 7
    if variant == 1 and cap == 1:
        same(host_entry(dec, relay, syn), rows_of(want, relay, slice(0, 400)), f"{what}, host entry")
        assert dec.info().last_grid == 1
    dec.close()


C240_CASES = [(relay, variant, cap) for relay in (False, True) for variant, cap in ((1, 1), (1, 3), (2, 1))]


@pytest.mark.parametrize("relay,variant,cap", C240_CASES,
                         ids=[f"{'relay' if r else 'minsum'}-tier{v}-grid{c}" for r, v, c in C240_CASES])
def test_240_8_4_nine_tiles_of_16_under_a_capped_grid(ldpc, gpu, monkeypatch, relay, variant, cap):
    case = c240_reuse_case(relay)
    syn, want = case[2], case[6]
    S = 16 if variant == 1 else 64
    dec = capped_decoder(ldpc, monkeypatch, cap, relay, case, variant)
    assert (dec.info().kernel, dec.info().tile_syndromes) == (variant, S)
    what = f"{'relay' if relay else 'min-sum'} (240,8,4) tier {variant} grid {cap}"
    same(device_entry(dec, relay, syn), rows_of(want, relay, slice(0, 130)), what)
    assert dec.info().last_grid == cap < tiles_of(130, S) == (9 if variant == 1 else 3)
    same(device_entry(dec, relay, syn[100:130]), rows_of(want, relay, slice(100, 130)), what + ", columns 100:130")
    assert dec.info().last_grid == min(cap, tiles_of(30, S))
    dec.close()


# ---- c. a second tile in the same slot, product build, no knob --------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("kind", ["minsum", "relay9", "relay3"])
def test_bb72_more_tiles_than_resident_workgroups_in_the_product_build(ldpc, gpu, monkeypatch, kind, variant):
    """64 (2 CUs + 1) + 37 syndromes: the 400 known ones repeated with a roll of 13 per repetition, so that equal syndromes
    sit in other lanes and tiles; the expected output is the model's 400 results indexed the same way.  The grid must
    come out smaller than the tile count -- if the occupancy of the kernels ever makes that false, this fails."""
    import torch

    monkeypatch.delenv("LDPC_MS_GRID_MAX", raising=False)
    assert not ldpc._capi.knobs_in_env()
    relay = kind != "minsum"
    H, prior, syn, g, legs, stop_after, want = bb72_reuse_case(kind)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 * (2 * cus + 1) + 37
    b = np.arange(B)
    idx = (b + 13 * (b // 400)) % 400
    assert idx[400] == 13 and (idx[:400] == np.arange(400)).all()
    dec = make_decoder(ldpc, relay, H, prior, g, legs, variant=variant, stop_after=stop_after)
    assert dec._L is ldpc._capi.lib(False) and (dec.info().kernel, dec.info().tile_syndromes) == (variant, 64)
    got = device_entry(dec, relay, syn[idx])
    info = dec.info()
    print(f"{kind} tier {variant}: {cus} CUs, batch {B}, tiles {tiles_of(B, 64)}, last_grid {info.last_grid}")
    assert 0 < info.last_grid < tiles_of(B, 64), (info, B)
    same(got, rows_of(want, relay, idx), f"{kind} tier {variant}, batch {B}")
    dec.close()


# ---- d. two handles of different widths alive together ---------------------------------------------------------------

@pytest.mark.parametrize("relay", [False, True], ids=["minsum", "relay"])
def test_handles_of_width_64_and_1_alive_together(ldpc, gpu, relay):
    """Both kernels raise the dynamic-LDS limit per kernel, not per handle: the S = 64 handle (min-sum: n = 96 of the table;
    relay, whose table has no on-chip row of 64: BB-72 H_X) and the S = 1 handle (n = 6144 / 3072) decode alternately,
    then the wide one is closed and the narrow one decodes once more."""
    if relay:
        w, narrow = bb72_reuse_case("relay3"), width_case(True, 3072, 1)
        wide = (w[0], w[1], w[2], w[3], w[4], w[6])
        dec_w = make_decoder(ldpc, True, w[0], w[1], w[3], w[4], stop_after=w[5])
    else:
        wide, narrow = width_case(False, 96, 64), width_case(False, 6144, 1)
        dec_w = make_decoder(ldpc, False, wide[0], wide[1], wide[3], wide[4])
    dec_n = make_decoder(ldpc, relay, narrow[0], narrow[1], narrow[3], narrow[4])
    assert (dec_w.info().kernel, dec_w.info().tile_syndromes) == (1, 64)
    assert (dec_n.info().kernel, dec_n.info().tile_syndromes) == (1, 1)
    Bw, Bn = min(wide[2].shape[0], 165), narrow[2].shape[0]
    for turn in range(2):
        same(device_entry(dec_w, relay, wide[2][:Bw]), rows_of(wide[5], relay, slice(0, Bw)), f"S 64, turn {turn}")
        assert dec_w.info().last_grid == tiles_of(Bw, 64)
        same(device_entry(dec_n, relay, narrow[2]), rows_of(narrow[5], relay, slice(0, Bn)), f"S 1, turn {turn}")
        assert dec_n.info().last_grid == Bn
    dec_w.close()
    same(device_entry(dec_n, relay, narrow[2]), rows_of(narrow[5], relay, slice(0, Bn)), "S 1 after the S 64 handle was closed")
    dec_n.close()
