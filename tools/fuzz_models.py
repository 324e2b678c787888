#!/usr/bin/env python3
"""Randomised model-parity fuzz (GPU box) of the kernels that tools/fuzz_parity.py does not reach: the bit-flip decoder,
min-sum (flooding and layered schedule, shared and per-syndrome priors), relay min-sum, the joint X/Z (Pauli) min-sum, the
device OSD step, the one-matrix and CSS trial steps, the three BP-OTS kernels at parameters fuzz_parity.py leaves out, the Pauli relay min-sum, the OSD step by the
standard rule, the stabilizer (non-CSS) min-sum, and the guided-decimation min-sum (leg `decim`: 2 ... 4 model seconds for the 40 cases of seeds 20 and 21).  Random Tanner graphs (irregular with empty and heavy nodes and
sizes around the word boundaries, or small Gallager codes), ragged batches, every `kernel_variant` that create accepts,
every result compared in every element with the numpy models of tests/ (the min-sum family and relay: the LLR bit patterns
too).  Usage: fuzz_models.py [cases] [seed] -- count-based: a seed names a fixed set of cases.

FUZZ_DRY=1: draw the cases and print them without touching the GPU or a model (no draw depends on a result, so this lists
what a run with the same seed decodes); FUZZ_FROM / FUZZ_TO: only run the cases with these indices (the others are drawn
and skipped); FUZZ_VERBOSE=1: one line per leg BEFORE it runs; FUZZ_MODEL_ONLY=1: no GPU, the models alone, with their
seconds.  A leg is skipped only when create answers UNSUPPORTED for an on-chip tier; every component decodes every case on
its unlimited tier.  The leg in hand is kept in fuzz_models_current.txt and, on a mismatch (exit status 1), the inputs in
fuzz_models_failure.npz, both in the directory FUZZ_OUT (default: fuzz_out/ in the repository root, which git ignores).

The legs `layered`, `priors` and `pauli` draw from a generator of their own (seeded [seed, 1]): the six older legs decode for
a seed what they decoded before those three existed.  The leg `bpots` draws from a third (seeded [seed, 2]) for the same
reason, and the leg `decim` (guided-decimation min-sum) from a fourth (seeded [seed, 3]); its line ends with `n` and the
on-chip tile width of the unforced plan (`S 0`: nothing fits on chip), which draw nothing.  BP-OTS has no kernel_variant: its tiers are the kernels 2 (LDS-resident), 3 (node-parallel) and 5 (unlimited), reached
through LDPC_BPOTS_FORCE_NODE unset, 1 and 2 (experiments build); a graph with a check of more than 32 or a bit of more than
16 edges runs as kernel 5 only and the other two count as skipped.  Its model is the C oracle (oracle/bpots_oracle.c), its
batch is capped at 65.

Model seconds of 40 cases on one CPU core (the `model seconds` line of FUZZ_MODEL_ONLY=1, all ten legs in one run): the six older
legs, the three of the second generator, and the BP-OTS oracle (C, not numpy):
  seed 20: bitflip 0.43, minsum 2.64, relay 5.82, osd 0.84, trials 0.06, css 0.08 (9.9 s); layered 1.68, priors 2.05, pauli 2.59 (6.3 s); bpots 2.04
  seed 21: bitflip 0.34, minsum 1.92, relay 4.96, osd 0.69, trials 0.06, css 0.08 (8.1 s); layered 1.56, priors 1.60, pauli 1.84 (5.0 s); bpots 1.42

The legs `pauli_relay` (the Pauli relay min-sum: Hx the case's graph, Hz a second drawn matrix, a count of its own for every
leg) and `osd_search` (the OSD step by the standard rule: combination sweep or exhaustive search, Hamming cost or weights)
draw from a fifth and a sixth generator (seeded [seed, 4] and [seed, 5]): the eleven older legs draw what they drew.  The
batch of `osd_search` is capped at 65, so that its model costs no more than the relay leg's for the same seed.  Model
seconds of these two legs for 40 cases, all thirteen legs in one run on one core of a faster machine than the figures
above come from, with the relay leg of the same run beside them:
  seed 20: pauli_relay 3.59, osd_search 0.92 (relay 2.67)
  seed 21: pauli_relay 3.04, osd_search 1.01 (relay 2.26)

The leg `stab` (the joint Pauli min-sum of a general stabilizer code: Sx the case's graph, Sz a second drawn pattern of the
same shape, an edge both store is Y-type; the rows need not commute) draws from a seventh generator (seeded [seed, 6]): the
thirteen older legs draw what they drew.  Its batch is capped at 65 and its second pattern is sparser than the case's, so
that the model, which walks the union graph, costs less than the relay leg's.  Model seconds for 40 cases, all fourteen
legs in one run on one core, with the relay leg of the same run beside them:
  seed 20: stab 1.91 (relay 3.03)
  seed 21: stab 1.76 (relay 2.49)"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # the models are test infrastructure
import ldpcdecoders_jl_amd as ldpc  # noqa: E402
import css_trials_model as cm  # noqa: E402
import dem_model as dm  # noqa: E402
import trials_model as tm  # noqa: E402
import priors_model as pm  # noqa: E402
from bitflip_model import BitFlipModel  # noqa: E402
from layered_model import LayeredMinSumModel, layers_of  # noqa: E402
from decim_model import DecimModel  # noqa: E402
from minsum_model import MinSumModel, llr_of_probs  # noqa: E402
from osd_model import osd_model_postprocess  # noqa: E402
from osd_search_model import METHODS as OSD_SEARCH_METHODS, osd_search_model, weights_of as osd_search_weights_of  # noqa: E402
from pauli_model import PauliMinSumModel, pauli_priors  # noqa: E402
from pauli_relay_model import PauliRelayModel  # noqa: E402
from relay_model import RelayModel  # noqa: E402
from stab_model import StabMinSumModel  # noqa: E402
from oracle import BPOTSOracle  # noqa: E402

DRY = os.environ.get("FUZZ_DRY") == "1"
FROM, TO = int(os.environ.get("FUZZ_FROM", "0")), int(os.environ.get("FUZZ_TO", str(1 << 60)))
VERBOSE = os.environ.get("FUZZ_VERBOSE") == "1"
MODEL_ONLY = os.environ.get("FUZZ_MODEL_ONLY") == "1"
GPU = not (DRY or MODEL_ONLY)
OUT = os.environ.get("FUZZ_OUT") or os.path.join(ROOT, "fuzz_out")
UNSUPPORTED = 5
# tiers a component can take here; the last one is its unlimited tier.  (Bit-flip tier 4, the 64-bit votes, needs
# max_iters * max bit degree >= 2^31 and is held by test_unlimited_tier_with_64_bit_votes.)
TIERS = {"bitflip": (1, 2, 3), "minsum": (1, 2), "relay": (1, 2), "osd": (1, 2, 3), "trials": (1, 2), "css": (1, 2),
         "layered": (1, 2), "priors": (1, 2), "pauli": (1, 2), "bpots": (2, 3, 5), "decim": (1, 2), "pauli_relay": (1, 2),
         "osd_search": (1, 2, 3), "stab": (1, 2)}
BOUNDARY = (31, 32, 33, 63, 64, 65, 127, 128, 129)

if GPU:
    import torch

    # every host-side wait of the library is bounded (host_wait.hpp): on these small graphs no leg needs more than
    # seconds, so a stall names itself after 40 s instead of sitting silent until the runner's limit
    for exp_build in (False, True):
        ldpc._capi.check(ldpc._capi.lib(exp_build).ldpc_set_wait_limit_ms(int(os.environ.get("FUZZ_WAIT_LIMIT_MS", "40000"))),
                         ldpc._capi.lib(exp_build))

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
rng2 = np.random.default_rng([seed, 1])      # the layered, priors and pauli legs: never `rng`, whose stream the older legs own
rng3 = np.random.default_rng([seed, 2])      # the bpots leg
rng4 = np.random.default_rng([seed, 3])      # the decim leg
rng5 = np.random.default_rng([seed, 4])      # the pauli_relay leg
rng6 = np.random.default_rng([seed, 5])      # the osd_search leg
rng7 = np.random.default_rng([seed, 6])      # the stab leg
t0 = time.time()
ran = {c: set() for c in TIERS}          # tiers that decoded
legs_run = {c: 0 for c in TIERS}
skipped = {c: 0 for c in TIERS}
model_s = {c: 0.0 for c in TIERS}
case = -1


def note(component, text):
    """What is about to run, where a run that stalls leaves it behind."""
    if VERBOSE:
        print(f"   {component}: {text}", flush=True)
    try:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "fuzz_models_current.txt"), "w") as fh:
            fh.write(f"seed {seed} case {case} after {time.time() - t0:.0f} s: {component}: {text}\n")
    except OSError:
        pass


def fail(component, text, **arrays):
    try:
        os.makedirs(OUT, exist_ok=True)
        np.savez(os.path.join(OUT, "fuzz_models_failure.npz"), component=component, text=text, seed=seed, case=case,
                 **{k: np.asarray(v) for k, v in arrays.items() if v is not None})
    except OSError:
        pass
    print(f"MISMATCH seed {seed} case {case} {component}: {text}", flush=True)
    sys.exit(1)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def same_bits(llr64, model32):
    """The library's float64 LLRs against the model's float32 ones, as bit patterns."""
    return llr64.dtype == np.float64 and np.array_equal(llr64.view(np.int64), model32.astype(np.float64).view(np.int64))


def timed_model(component, f):
    t = time.time()
    out = f()
    model_s[component] += time.time() - t
    return out


def on_every_tier(component, variants, create, run, text, tier_of=lambda h: int(h.kernel)):
    """create(variant) -> handle (LdpcError UNSUPPORTED for an on-chip tier: the leg is skipped); run(handle, tier)
    compares; the unlimited tier must run.  tier_of(handle): the tier that the entries under test take; 0 = they are
    unsupported on this handle, which for an on-chip variant is a skipped leg as well."""
    unlimited = TIERS[component][-1]
    for variant in variants:
        note(component, f"kernel_variant {variant} {text}")
        try:
            h = create(variant)
        except ldpc.LdpcError as e:
            if e.status == UNSUPPORTED and variant != unlimited:
                skipped[component] += 1
                continue
            raise
        tier = tier_of(h)
        if tier == 0 and variant != unlimited:
            h.close()
            skipped[component] += 1
            continue
        if tier != variant:
            fail(component, f"kernel_variant {variant} gave tier {tier} {text}")
        run(h, variant)
        h.close()
        ran[component].add(tier)
        legs_run[component] += 1
        if variant == unlimited:
            break
    else:
        fail(component, f"the unlimited tier did not run {text}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A [rows][cols] uint8 device array at byte offset `off` inside a larger buffer of guard bytes."""

    def __init__(self, rows, cols, off, fill=0xA5):
        self.off, self.size, self.fill = int(off), rows * cols, fill
        self.buf = torch.full((self.off + self.size + 64,), fill, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.off:self.off + self.size].view(rows, cols)

    def put(self, a):
        self.view.copy_(dev(np.ascontiguousarray(a, dtype=np.uint8)))
        return self.view

    def guards_intact(self):
        return bool((self.buf[:self.off] == self.fill).all()) and bool((self.buf[self.off + self.size:] == self.fill).all())

    def get(self):
        return self.view.cpu().numpy()


# ---- the draws ---------------------------------------------------------------------------------------------------------
def draw_graph():
    kind = int(rng.integers(0, 4))
    if kind == 3:      # a small Gallager code
        wr, wc = int(rng.choice([4, 6, 8])), int(rng.choice([2, 3, 4]))
        n = wr * int(rng.integers(4, 40))
        H = ldpc.codes.parity_check_csc(n, wr, wc, seed=int(rng.integers(1 << 30)))
    else:              # irregular, with empty and heavy nodes and sizes at the word boundaries now and then
        s, n = int(rng.integers(1, 81)), int(rng.integers(1, 161))
        if rng.random() < 0.35:
            n = int(rng.choice(BOUNDARY))
        if rng.random() < 0.25:
            s = int(rng.choice(BOUNDARY[:6]))
        A = (rng.random((s, n)) < rng.uniform(0.02, 0.25)).astype(np.uint8)
        if rng.random() < 0.3:
            A[rng.integers(0, s), :] = 0
        if rng.random() < 0.3:
            A[:, rng.integers(0, n)] = 0
        if rng.random() < 0.3 and n >= 33:        # a row of 33 ... 80 ones
            A[rng.integers(0, s), rng.choice(n, size=min(n, int(rng.integers(33, 81))), replace=False)] = 1
        if rng.random() < 0.3 and s >= 20:        # a column of 20 ... s ones
            k = s if rng.random() < 0.4 else int(rng.integers(20, s + 1))
            A[rng.choice(s, size=k, replace=False), rng.integers(0, n)] = 1
        H = sp.csc_matrix(A)
    H.sort_indices()
    return kind, H


def draw_syndromes(H, B, g=None):
    """Syndromes of random errors, or arbitrary ones."""
    g = g or rng
    s, n = H.shape
    if g.random() < 0.6:
        return ldpc.codes.syndromes_of(H, (g.random((B, n)) < g.uniform(0.01, 0.2)).astype(np.uint8))
    return g.integers(0, 2, (B, s)).astype(np.uint8)


def draw_priors(shape, g=None):
    """Prior LLRs ([n], or [B][n] for a prior per syndrome) with a few negative, +-0 and subnormal ones."""
    g = g or rng
    prior = llr_of_probs(g.uniform(0.005, 0.45, shape))
    for value in (None, 0.0, -0.0, 1e-40, -1e-41):
        hit = g.random(shape) < 0.04
        prior[hit] = -prior[hit] if value is None else np.float32(value)
    return prior


# ---- the legs ----------------------------------------------------------------------------------------------------------
def leg_bitflip(H, B, run):
    s, n = H.shape
    rule = int(rng.integers(0, 3))
    bf_seed = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    max_iters = int(rng.choice([0, 1, 5, 30]))
    column0 = int(rng.choice([0, 5, (1 << 32) + 7, 1 << 40]))
    device_entry = bool(rng.random() < 0.5)
    syn = draw_syndromes(H, B)
    if rng.random() < 0.25:
        hit = rng.random(syn.shape) < 0.05
        syn[hit] = rng.integers(2, 4, size=int(hit.sum()))
    text = f"rule {rule} seed {bf_seed} max_iters {max_iters} column0 {column0} {'device' if device_entry else 'host'} entry"
    if DRY or VERBOSE:
        print(f"   bitflip {text}", flush=True)
    if not run:
        return
    want = timed_model("bitflip", lambda: BitFlipModel(H, max_iters).decode_batch(syn, rule, seed=bf_seed, column0=column0))
    if not GPU:
        return

    def go(dec, variant):
        if device_entry:
            err = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
            conv, stop = torch.full((B,), 9, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.uint8, device="cuda")
            its = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            dec.decode_batch_device(dev(syn), err, conv, its, stop, column0=column0)
            torch.cuda.synchronize()
            got = tuple(x.cpu().numpy() for x in (err, conv, its, stop))
        else:
            got = dec.decode_batch_host(syn, column0=column0)
        for name, g, w in zip(("errors", "converged", "iters", "stop_reason"), got, want):
            if not same(g, w):
                fail("bitflip", f"{name} differ, kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape,
                     syn=syn, got=g, want=w)

    on_every_tier("bitflip", (1, 2, 3), lambda v: ldpc.BitFlipDecoder(H, 0.01, max_iters, tie_break=rule, seed=bf_seed, kernel_variant=v),
                  go, text)


def leg_minsum(H, B, run):
    s, n = H.shape
    alpha, clip = float(rng.choice([0.5, 0.75, 1.0])), float(rng.choice([4.0, 20.0, 1e6]))
    max_iters = int(rng.choice([0, 1, 3, 20]))
    prior = draw_priors(n)
    device_entry = bool(rng.random() < 0.5)
    syn = draw_syndromes(H, B)
    text = f"alpha {alpha} clip {clip} max_iters {max_iters} {'device' if device_entry else 'host'} entry"
    if DRY or VERBOSE:
        print(f"   minsum {text}", flush=True)
    if not run:
        return
    merr, mconv, mits, mL = timed_model("minsum", lambda: MinSumModel(H, prior, max_iters, alpha=alpha, clip=clip).decode(syn))
    if not GPU:
        return

    def go(dec, variant):
        if device_entry:
            err, conv = torch.full((B, n), 7, dtype=torch.uint8, device="cuda"), torch.full((B,), 7, dtype=torch.uint8, device="cuda")
            llr = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda")
            its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            dec.decode_batch_device(dev(syn), err, conv, llr, its)
            torch.cuda.synchronize()
            err, conv, llr, its = (x.cpu().numpy() for x in (err, conv, llr, its))
        else:
            err, conv, llr, its = dec.decode_batch_host(syn, want_llr=True)
        ok = same(err, merr) and same(conv, mconv) and same(its, mits) and same_bits(llr, mL)
        if not ok:
            fail("minsum", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, prior=prior,
                 err=err, conv=conv, its=its, llr=llr, merr=merr, mconv=mconv, mits=mits, mL=mL)

    on_every_tier("minsum", (1, 2), lambda v: ldpc.MinSumDecoder(H, None, max_iters, channel_llr=prior, alpha=alpha, clip=clip, kernel_variant=v),
                  go, text)


class RelayPerLeg(ldpc.RelayMinSumDecoder):
    """A RelayMinSumDecoder with an iteration count of its own for every leg: ldpc_relay_create takes one per leg, the
    class's constructor gives leg 0 one count and all later legs another.  The decode methods are the class's."""

    def __init__(self, H, prior, gammas, leg_iters, stop_after, alpha, clip, kernel_variant):
        import ctypes

        capi = ldpc._capi
        M = ldpc.decoder._pattern_of(H)
        self.s, self.n, self.sparse_H = int(M.shape[0]), int(M.shape[1]), M
        self.channel_llr = np.ascontiguousarray(prior, dtype=np.float32)
        self.gammas = np.ascontiguousarray(gammas, dtype=np.float32)
        self.leg_iters = np.ascontiguousarray(leg_iters, dtype=np.int32)
        self.legs = int(self.leg_iters.size)
        assert self.channel_llr.shape == (self.n,) and self.gammas.shape == (self.legs, self.n)
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64)
        opts = capi.RelayOptions()
        opts.device = 0
        opts.alpha, opts.clip = float(alpha), float(clip)
        opts.kernel_variant, opts.stop_after = int(kernel_variant), int(stop_after)
        self.device = 0
        self._h = ctypes.c_void_p()
        self._L = capi.lib_for(None)
        capi.check(self._L.ldpc_relay_create(self.s, self.n, int(rowval.size), colptr.ctypes.data, rowval.ctypes.data,
                                             self.channel_llr.ctypes.data, self.legs, self.gammas.ctypes.data,
                                             self.leg_iters.ctypes.data, ctypes.byref(opts), ctypes.byref(self._h)), self._L)


def leg_relay(H, B, run):
    s, n = H.shape
    legs = int(rng.integers(1, 5))
    leg_iters = [int(x) for x in rng.integers(0, 9, size=legs)]      # a leg of 0 iterations is skipped, wherever it stands
    gammas = rng.uniform(-0.3, 0.9, size=(legs, n)).astype(np.float32)
    stop_after = int(rng.integers(1, 4))
    alpha, clip = float(rng.choice([0.5, 0.75, 1.0])), float(rng.choice([4.0, 20.0, 1e6]))
    prior = draw_priors(n)
    device_entry, want_solutions = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    syn = draw_syndromes(H, B)
    text = (f"leg_iters {leg_iters} stop_after {stop_after} alpha {alpha} clip {clip} {'device' if device_entry else 'host'} entry "
            f"solutions={want_solutions}")
    if DRY or VERBOSE:
        print(f"   relay {text}", flush=True)
    if not run:
        return
    merr, mconv, mits, msol, mM = timed_model(
        "relay", lambda: RelayModel(H, prior, gammas, leg_iters, alpha=alpha, clip=clip, stop_after=stop_after).decode(syn))
    if not GPU:
        return

    def go(dec, variant):
        if device_entry:
            err, conv = torch.full((B, n), 7, dtype=torch.uint8, device="cuda"), torch.full((B,), 7, dtype=torch.uint8, device="cuda")
            llr = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda")
            its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            sol = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_solutions else None
            dec.decode_batch_device(dev(syn), err, conv, llr, its, sol)
            torch.cuda.synchronize()
            err, conv, llr, its = (x.cpu().numpy() for x in (err, conv, llr, its))
            sol = sol.cpu().numpy() if want_solutions else None
        else:
            out = dec.decode_batch_host(syn, want_llr=True, want_solutions=want_solutions)
            err, conv, llr, its = out[:4]
            sol = out[4] if want_solutions else None
        ok = same(err, merr) and same(conv, mconv) and same(its, mits) and same_bits(llr, mM) and (sol is None or same(sol, msol))
        if not ok:
            fail("relay", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, prior=prior,
                 gammas=gammas, leg_iters=leg_iters, err=err, conv=conv, its=its, llr=llr, sol=sol, merr=merr, mconv=mconv, mits=mits,
                 msol=msol, mM=mM)

    on_every_tier("relay", (1, 2), lambda v: RelayPerLeg(H, prior, gammas, leg_iters, stop_after, alpha, clip, v), go, text)


def leg_osd(H, B, run):
    s, n = H.shape
    order = int(rng.integers(0, 9))
    inplace = bool(rng.random() < 0.5)
    Bo = min(B, 65)      # (the model is one dense elimination and 2^order candidates per syndrome)
    # consistent syndromes only: the estimate for a syndrome outside the column space of H is not specified
    syn = ldpc.codes.syndromes_of(H, (rng.random((Bo, n)) < 0.1).astype(np.uint8))
    bp_err = (rng.random((Bo, n)) < 0.1).astype(np.uint8)
    llr = -np.exp(rng.uniform(-8, 1, (Bo, n)))
    llr[rng.random((Bo, n)) < 0.3] = llr[0, 0]       # ties
    if rng.random() < 0.3:
        llr[rng.random((Bo, n)) < 0.05] = np.nan
        llr[rng.random((Bo, n)) < 0.03] = -np.inf
        llr[rng.random((Bo, n)) < 0.03] = np.inf
    text = f"order {order} batch {Bo} {'in place' if inplace else 'out of place'}"
    if DRY or VERBOSE:
        print(f"   osd {text}", flush=True)
    if not run:
        return
    Hd = np.asarray(H.todense()).astype(np.uint8)
    want = timed_model("osd", lambda: np.stack([osd_model_postprocess(Hd, syn[b], bp_err[b], llr[b], order) for b in range(Bo)]))
    if not GPU:
        return

    class Post:
        def __init__(self, variant):
            self.post = ldpc.OSDPostProcessor(H, order)
            try:
                self.post.prepare_device(0, variant)
            except ldpc.LdpcError:
                self.post.close()
                raise
            self.kernel = self.post.kernel

        def close(self):
            self.post.close()

    def go(h, variant):
        d_err = dev(bp_err)
        out = h.post.postprocess_device(dev(syn), d_err, dev(llr), out=d_err if inplace else None)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if not same(got, want) or not (inplace or same(d_err.cpu().numpy(), bp_err)):
            fail("osd", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, bp_err=bp_err,
                 llr=llr, got=got, want=want)

    on_every_tier("osd", (1, 2, 3), Post, go, text)


def draw_offsets(k):
    return [int(x) for x in rng.integers(0, 16, size=k)]


def leg_trials(H, B, run):
    s, n = H.shape
    nl = int(rng.integers(0, 6))
    L = sp.csc_matrix((rng.random((nl, n)) < rng.uniform(0.05, 0.5)).astype(np.uint8)) if nl else None
    per = float(rng.choice([0.0, 1.0, 1e-12, 0.02, 0.3, 0.5]))
    rates = rng.uniform(0.0, 1.0, n) ** 3
    rates[rng.random(n) < 0.1] = 0.0
    rates[rng.random(n) < 0.1] = 1.0
    rates[rng.random(n) < 0.1] = 1e-12
    tr_seed = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    column0 = int(rng.choice([0, 3, (1 << 32) + 1, 1 << 40]))
    given = rng.integers(0, 2, (B, n)).astype(np.uint8)
    if rng.random() < 0.3:
        given |= (rng.integers(0, 128, (B, n)) << 1).astype(np.uint8)      # only the low bit of an error byte counts
    guesses = given ^ (rng.random((B, n)) < rng.choice([0.0, 0.01, 0.2])).astype(np.uint8)
    exact = rng.random(B) < 0.3
    guesses[exact] = given[exact]
    offs = draw_offsets(7)
    text = f"nl {nl} per {per} seed {tr_seed} column0 {column0} offsets {offs}"
    if DRY or VERBOSE:
        print(f"   trials {text}", flush=True)
    if not run:
        return

    def models():
        e1 = tm.sample(n, B, per, tr_seed, column0)
        e2 = dm.sample(rates, B, tr_seed, column0)
        return e1, tm.syndromes(H, e1), e2, tm.syndromes(H, e2), tm.syndromes(H, given), tm.score(H, L, guesses, given)

    e1, s1, e2, s2, s3, (flags, counts) = timed_model("trials", models)
    if not GPU:
        return

    def go(t, variant):
        def check(what, got, want, *bufs):
            if not same(got, want) or not all(b.guards_intact() for b in bufs):
                fail("trials", f"{what}, kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape,
                     logicals=L.todense() if L is not None else None, rates=rates, given=given, guesses=guesses, got=got, want=want)

        be, bs = Guarded(B, n, offs[0]), Guarded(B, s, offs[1])
        t.sample(B, per, seed=tr_seed, column0=column0, out=(be.view, bs.view))
        check("sample errors", be.get(), e1, be, bs)
        check("sample syndromes", bs.get(), s1, be, bs)
        be, bs = Guarded(B, n, offs[2]), Guarded(B, s, offs[3])
        t.set_rates(rates)
        t.sample_rates(B, seed=tr_seed, column0=column0, out=(be.view, bs.view))
        check("sample_rates errors", be.get(), e2, be, bs)
        check("sample_rates syndromes", bs.get(), s2, be, bs)
        bg, bs = Guarded(B, n, offs[4]), Guarded(B, s, offs[3])
        t.syndromes(bg.put(given), out=bs.view)
        check("syndromes of given errors", bs.get(), s3, bg, bs)
        bq, bf = Guarded(B, n, offs[5]), Guarded(B, 1, offs[6])
        start = torch.tensor([5, 6, 7, 8], dtype=torch.int64, device="cuda")       # counts are accumulated into
        _, c = t.score(bq.put(guesses), bg.view, flags=bf.view.view(B), counts=start)
        check("score flags", bf.get().reshape(B), flags, bq, bg, bf)
        check("score counts", c.cpu().numpy() - np.array([5, 6, 7, 8]), counts)

    on_every_tier("trials", (1, 2), lambda v: ldpc.Trials(H, L, kernel_variant=v), go, text)


def leg_css(B, run):
    """The hypergraph product of two drawn small matrices."""
    def small():
        r, c = int(rng.integers(1, 5)), int(rng.integers(2, 7))
        return (rng.random((r, c)) < 0.5).astype(np.uint8)

    Hx, Hz = ldpc.codes.hypergraph_product(small(), small())
    n = Hx.shape[1]
    with_logicals = bool(rng.random() < 0.7)
    p = [0.0, 0.05, 0.9, (0.01, 0.002, 0.03), (0.0, 0.0, 0.4), (0.3, 0.3, 0.3)][int(rng.integers(0, 6))]
    tr_seed = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    column0 = int(rng.choice([0, 3, (1 << 32) + 1, 1 << 40]))
    gex, gez = rng.integers(0, 2, (B, n)).astype(np.uint8), rng.integers(0, 2, (B, n)).astype(np.uint8)
    flip = float(rng.choice([0.0, 0.01, 0.2]))
    gx, gz = gex ^ (rng.random((B, n)) < flip).astype(np.uint8), gez ^ (rng.random((B, n)) < flip).astype(np.uint8)
    offs = draw_offsets(10)
    text = f"css Hx {Hx.shape} Hz {Hz.shape} logicals={with_logicals} p {p} seed {tr_seed} column0 {column0} offsets {offs}"
    if DRY or VERBOSE:
        print(f"   {text}", flush=True)
    if not run:
        return
    Lx, Lz = ldpc.codes.css_logicals(Hx, Hz) if with_logicals else (None, None)

    def models():
        ex, ez = cm.sample(n, B, p, tr_seed, column0)
        return ex, ez, cm.syndromes(Hx, Hz, ex, ez), cm.syndromes(Hx, Hz, gex, gez), cm.score(Hx, Hz, Lx, Lz, gx, gz, gex, gez)

    ex, ez, (sx, sz), (gsx, gsz), (flags, counts) = timed_model("css", models)
    if not GPU:
        return
    rx, rz = Hx.shape[0], Hz.shape[0]

    def go(t, variant):
        def check(what, got, want, *bufs):
            if not same(got, want) or not all(b.guards_intact() for b in bufs):
                fail("css", f"{what}, kernel_variant {variant} {text}", hx=Hx.todense(), hz=Hz.todense(), gex=gex, gez=gez, gx=gx, gz=gz,
                     got=got, want=want)

        b = [Guarded(B, n, offs[0]), Guarded(B, n, offs[1]), Guarded(B, rx, offs[2]), Guarded(B, rz, offs[3])]
        t.sample(B, p, seed=tr_seed, column0=column0, out=tuple(x.view for x in b))
        for what, buf, want in zip(("ex", "ez", "sx", "sz"), b, (ex, ez, sx, sz)):
            check("sample " + what, buf.get(), want, *b)
        be = [Guarded(B, n, offs[4]), Guarded(B, n, offs[5])]
        bs = [Guarded(B, rx, offs[3]), Guarded(B, rz, offs[2])]
        t.syndromes(be[0].put(gex), be[1].put(gez), out=(bs[0].view, bs[1].view))
        check("syndromes sx", bs[0].get(), gsx, *be, *bs)
        check("syndromes sz", bs[1].get(), gsz, *be, *bs)
        bg = [Guarded(B, n, offs[6]), Guarded(B, n, offs[7])]
        bf = Guarded(B, 1, offs[8])
        start = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int64, device="cuda")
        _, c = t.score(bg[0].put(gx), bg[1].put(gz), be[0].view, be[1].view, flags=bf.view.view(B), counts=start)
        check("score flags", bf.get().reshape(B), flags, *bg, *be, bf)
        check("score counts", c.cpu().numpy() - np.arange(1, 7), counts)

    logicals = (Lx, Lz) if with_logicals else False
    on_every_tier("css", (1, 2), lambda v: ldpc.CSSTrials(Hx, Hz, logicals, kernel_variant=v), go, text)


# ---- the legs of the second generator ----------------------------------------------------------------------------------
def draw_rule(g):
    """alpha, clip, max_iters of a leg of the min-sum family (the models loop over the edges in Python: 10 iterations)."""
    return float(g.choice([0.5, 0.75, 1.0])), float(g.choice([4.0, 20.0, 1e6])), int(g.choice([0, 1, 3, 10]))


def degrees_text(H, name):
    """The record forms among the checks of H (csc) and its empty checks, for a dry line."""
    deg = np.diff(sp.csr_matrix(H).indptr)
    return (f"{name}<=32 {int(((deg > 0) & (deg <= 32)).sum())} {name}33-64 {int(((deg > 32) & (deg <= 64)).sum())} "
            f"{name}>64 {int((deg > 64).sum())} {name}_empty {int((deg == 0).sum())}")


def device_outputs(B, n, planes, want_llr, want_iters):
    """(err-like [B][n] u8, conv, llr | None, iters | None) on the device, pre-filled with values no decode writes."""
    shape = (B, n) if planes == 1 else (B, planes, n)
    return (torch.full((B, n), 7, dtype=torch.uint8, device="cuda"), torch.full((B,), 7, dtype=torch.uint8, device="cuda"),
            torch.full(shape, 7.0, dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None)


def host_of(x):
    return None if x is None else x.cpu().numpy()


def leg_layered(H, B, run):
    g = rng2
    s, n = H.shape
    alpha, clip, max_iters = draw_rule(g)
    prior = draw_priors(n, g)
    device_entry = bool(g.random() < 0.5)
    syn = draw_syndromes(H, B, g)
    text = f"alpha {alpha} clip {clip} max_iters {max_iters} {'device' if device_entry else 'host'} entry"
    if DRY or VERBOSE:
        layer_of, K = layers_of(H)
        sizes = np.bincount(layer_of[layer_of >= 0], minlength=K)
        print(f"   layered {text} layers {K} smallest_layer {int(sizes.min()) if K else 0} {degrees_text(H, 'checks')}", flush=True)
    if not run:
        return
    model = LayeredMinSumModel(H, prior, max_iters, alpha=alpha, clip=clip)
    merr, mconv, mits, mL = timed_model("layered", lambda: model.decode(syn))
    if not GPU:
        return

    def go(dec, variant):
        if int(dec.layers) != model.K:
            fail("layered", f"{dec.layers} layers, the model has {model.K}, kernel_variant {variant} {text}", colptr=H.indptr,
                 rowval=H.indices, shape=H.shape)
        if device_entry:
            err, conv, llr, its = device_outputs(B, n, 1, True, True)
            dec.decode_batch_device(dev(syn), err, conv, llr, its)
            torch.cuda.synchronize()
            err, conv, llr, its = (x.cpu().numpy() for x in (err, conv, llr, its))
        else:
            err, conv, llr, its = dec.decode_batch_host(syn, want_llr=True)
        if not (same(err, merr) and same(conv, mconv) and same(its, mits) and same_bits(llr, mL)):
            fail("layered", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, prior=prior,
                 err=err, conv=conv, its=its, llr=llr, merr=merr, mconv=mconv, mits=mits, mL=mL)

    on_every_tier("layered", (1, 2), lambda v: ldpc.MinSumDecoder(H, None, max_iters, channel_llr=prior, alpha=alpha, clip=clip,
                                                                  kernel_variant=v, schedule="layered"), go, text)


def leg_priors(H, B, run):
    """The entries with a prior per syndrome and bit: both schedules, the priors as floats or selected by given bits."""
    g = rng2
    s, n = H.shape
    schedule = ("flooding", "layered")[int(g.integers(0, 2))]
    source = ("floats", "given")[int(g.integers(0, 2))]
    alpha, clip, max_iters = draw_rule(g)
    shared = draw_priors(n, g)                 # the handle's channel_llr: these entries never read it
    nonfinite = 0
    if source == "floats":
        pri = draw_priors((B, n), g)
        if g.random() < 0.3:                   # a NaN, a +inf or a -inf in a few rows: such a row is not decoded
            rows = g.choice(B, size=min(B, int(g.integers(1, 4))), replace=False)
            pri[rows, g.integers(0, n, size=rows.size)] = g.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=rows.size)
            nonfinite = int(rows.size)
        t0 = t1 = given = None
    else:
        t0, t1 = draw_priors(n, g), draw_priors(n, g)
        given = g.integers(0, 256, size=(B, n), dtype=np.uint8)
        pri = pm.select_priors(given, t0, t1)
    device_entry, want_llr, want_iters = (bool(g.random() < 0.5) for _ in range(3))
    syn = draw_syndromes(H, B, g)
    text = (f"{schedule} {source} alpha {alpha} clip {clip} max_iters {max_iters} {'device' if device_entry else 'host'} entry "
            f"llr={want_llr} iters={want_iters} nonfinite_rows {nonfinite}")
    if DRY or VERBOSE:
        print(f"   priors {text}", flush=True)
    if not run:
        return
    merr, mconv, mits, mL = timed_model("priors", lambda: pm.model_of(schedule, H, max_iters, alpha, clip).decode(syn, pri))
    if not GPU:
        return

    def go(dec, variant):
        if source == "given":
            dec.set_conditional_priors(t0, t1)
        extra = pri if source == "floats" else given
        if device_entry:
            err, conv, llr, its = device_outputs(B, n, 1, want_llr, want_iters)
            entry = dec.decode_batch_priors_device if source == "floats" else dec.decode_batch_given_device
            entry(dev(syn), dev(extra), err, conv, llr, its)
            torch.cuda.synchronize()
            err, conv, llr, its = (host_of(x) for x in (err, conv, llr, its))
        else:
            entry = dec.decode_batch_priors_host if source == "floats" else dec.decode_batch_given_host
            err, conv, llr, its = entry(syn, extra, want_llr=want_llr)
            if (llr is None) != (not want_llr):
                fail("priors", f"the host entry returns LLRs it was not asked for, or none, kernel_variant {variant} {text}")
        ok = same(err, merr) and same(conv, mconv) and (its is None or same(its, mits)) and (llr is None or same_bits(llr, mL))
        if not ok:
            fail("priors", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, pri=pri,
                 given=given, t0=t0, t1=t1, err=err, conv=conv, its=its, llr=llr, merr=merr, mconv=mconv, mits=mits, mL=mL)

    on_every_tier("priors", (1, 2), lambda v: ldpc.MinSumDecoder(H, None, max_iters, channel_llr=shared, alpha=alpha, clip=clip,
                                                                 kernel_variant=v, schedule=schedule), go, text,
                  tier_of=lambda h: int(h.info().priors_kernel))


def draw_pauli_probs(n, g):
    """(probs [n][3], uniform): per-qubit (px, py, pz); a few qubits where one Pauli is likelier than I (a negative prior), a
    few with pW == 1 - px - py - pz exactly (a prior of +0: 0.25 against 0.125 and 0.375, all exact in binary); in a quarter
    of the cases one triple (a, b, a) for every qubit, so that GX == GZ wherever TX == TZ."""
    if g.random() < 0.25:
        a, b = g.uniform(0.005, 0.1, size=2)
        return np.tile(np.array([a, b, a]), (n, 1)), True
    probs = g.uniform(0.002, 0.1, size=(n, 3))
    likely = np.nonzero(g.random(n) < 0.06)[0]
    probs[likely] = 0.1
    probs[likely, g.integers(0, 3, size=likely.size)] = g.uniform(0.4, 0.7, size=likely.size)
    zero = np.nonzero(g.random(n) < 0.06)[0]
    for j, w in zip(zero, g.integers(0, 3, size=zero.size)):
        probs[j] = np.roll([0.25, 0.125, 0.375], w)
    return probs, False


def draw_hz(n, g):
    """(A dense, Hz csc): a second matrix of 1 ... 40 rows over the n qubits of the case's graph, with an empty row and a row
    of 33 ... 80 ones now and then."""
    rz = int(g.integers(1, 41))
    A = (g.random((rz, n)) < g.uniform(0.02, 0.25)).astype(np.uint8)
    empty, heavy = int(g.integers(0, rz)), int(g.integers(0, rz))
    if heavy == empty:
        heavy = (heavy + 1) % rz
    if g.random() < 0.35:
        A[empty, :] = 0
    if g.random() < 0.5 and n >= 33:          # a row of 33 ... 80 ones
        A[heavy, g.choice(n, size=min(n, int(g.integers(33, 81))), replace=False)] = 1
    Hz = sp.csc_matrix(A)
    Hz.sort_indices()
    return A, Hz


def leg_pauli(H, B, run):
    """Hx = the case's H, Hz a second drawn matrix over the same qubits; the sides need not commute (check=False)."""
    g = rng2
    rx, n = H.shape
    A, Hz = draw_hz(n, g)
    rz = Hz.shape[0]
    alpha, clip, max_iters = draw_rule(g)
    probs, uniform = draw_pauli_probs(n, g)
    device_entry, want_llr, want_iters = (bool(g.random() < 0.5) for _ in range(3))
    sampled = bool(g.random() < 0.6)
    if sampled:                               # the syndromes of sampled Pauli errors: sx = Hx ez, sz = Hz ex
        rate = g.uniform(0.01, 0.15)
        ex, ez = ((g.random((B, n)) < rate).astype(np.uint8) for _ in range(2))
        sx, sz = ldpc.codes.syndromes_of(H, ez), ldpc.codes.syndromes_of(Hz, ex)
    else:
        sx, sz = g.integers(0, 2, (B, rx)).astype(np.uint8), g.integers(0, 2, (B, rz)).astype(np.uint8)
    text = (f"Hz ({rz}, {n}) B {B} alpha {alpha} clip {clip} max_iters {max_iters} {'device' if device_entry else 'host'} entry "
            f"llr={want_llr} iters={want_iters} uniform={uniform} {'sampled' if sampled else 'arbitrary'} syndromes")
    if DRY or VERBOSE:
        print(f"   pauli {text} {degrees_text(H, 'hx')} {degrees_text(Hz, 'hz')}", flush=True)
    if not run:
        return
    tables = pauli_priors(probs)
    mgx, mgz, mconv, mits, mG = timed_model(
        "pauli", lambda: PauliMinSumModel(H, Hz, tables, max_iters, alpha=alpha, clip=clip).decode(sx, sz))
    if not GPU:
        return

    def go(dec, variant):
        for name, got, want in zip("xyz", (dec.prior_x, dec.prior_y, dec.prior_z), tables):
            if not (got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))):
                fail("pauli", f"prior_{name} differs from the model's table {text}", probs=probs, got=got, want=want)
        if device_entry:
            gx, conv, llr, its = device_outputs(B, n, 3, want_llr, want_iters)
            gz = torch.full((B, n), 7, dtype=torch.uint8, device="cuda")
            dec.decode_batch_device(dev(sx), dev(sz), gx, gz, conv, llr, its)
            torch.cuda.synchronize()
            gx, gz, conv, llr, its = (host_of(x) for x in (gx, gz, conv, llr, its))
        else:
            gx, gz, conv, llr, its = dec.decode_batch_host(sx, sz, want_llr=want_llr)
        ok = (same(gx, mgx) and same(gz, mgz) and same(conv, mconv) and (its is None or same(its, mits))
              and (llr is None or same_bits(llr, mG)))
        if not ok:
            fail("pauli", f"kernel_variant {variant} {text}", hx_colptr=H.indptr, hx_rowval=H.indices, hx_shape=H.shape, hz=A, probs=probs,
                 sx=sx, sz=sz, gx=gx, gz=gz, conv=conv, its=its, llr=llr, mgx=mgx, mgz=mgz, mconv=mconv, mits=mits, mG=mG)

    on_every_tier("pauli", (1, 2), lambda v: ldpc.PauliMinSumDecoder(H, Hz, None, max_iters, pauli_probs=probs, alpha=alpha, clip=clip,
                                                                     kernel_variant=v, check=False), go, text)


# ---- the leg of the third generator ------------------------------------------------------------------------------------
BPOTS_BATCH_CAP = 65      # (the oracle costs about 0.28 us per edge, iteration and syndrome)


def leg_bpots(H, B, run):
    """The three BP-OTS kernels on the case's graph (graphs without edges included) against the C oracle: errors, flags and
    iteration counts in every element."""
    g = rng3
    s, n = H.shape
    per = float(g.choice([1e-6, 0.01, 0.05, 0.2, 0.75, 0.9]))
    T, C = int(g.choice([1, 2, 3, 9])), float(g.choice([0.0, 1.0, 2.0, 3.0]))
    max_iters = int(g.choice([0, 1, 3, 10]))
    device_entry, want_iters = bool(g.random() < 0.5), bool(g.random() < 0.5)
    Bo = min(B, BPOTS_BATCH_CAP)
    syn = draw_syndromes(H, Bo, g)
    if g.random() < 0.25:
        hit = g.random(syn.shape) < 0.05
        syn[hit] = g.integers(2, 4, size=int(hit.sum()))
    plans = [ldpc.bpots.bpots_plan_of(H, force_node=f) for f in (0, 1, 2)]      # host code: no device needed
    text = (f"per {per} T {T} C {C} max_iters {max_iters} batch {Bo} {'device' if device_entry else 'host'} entry iters={want_iters} "
            f"edges {H.nnz} kernel {plans[0].kernel} S {plans[0].S} DC {plans[0].DC} DV {plans[0].DV}")
    if DRY or VERBOSE:
        print(f"   bpots {text}", flush=True)
    if not run:
        return
    werr, wconv, wits = timed_model("bpots", lambda: BPOTSOracle((H.indptr, H.indices), H.shape, per, max_iters, T, C).batchdecode(syn))
    if not GPU:
        return
    done = set()
    for force, plan in enumerate(plans):
        if plan.kernel in done:          # a wide graph: LDPC_BPOTS_FORCE_NODE changes nothing
            skipped["bpots"] += 1
            continue
        note("bpots", f"LDPC_BPOTS_FORCE_NODE {force} {text}")
        if force:
            os.environ["LDPC_BPOTS_FORCE_NODE"] = str(force)
        try:
            dec = ldpc.BPOTSDecoder(H, per, max_iters, T=T, C=C)
        finally:
            os.environ.pop("LDPC_BPOTS_FORCE_NODE", None)
        if dec.kernel != plan.kernel:
            fail("bpots", f"LDPC_BPOTS_FORCE_NODE {force} gave kernel {dec.kernel}, the plan says {plan.kernel} {text}")
        if device_entry:
            err, conv, _, its = device_outputs(Bo, n, 1, False, want_iters)
            dec.decode_batch_device(dev(syn), err, conv, its)
            torch.cuda.synchronize()
            err, conv, its = (host_of(x) for x in (err, conv, its))
        else:
            err, conv, its = dec.decode_batch_host(syn)
        launch = dec.last_launch()
        dec.close()
        if not (same(err, werr) and same(conv, wconv) and (its is None or same(its, wits))):
            fail("bpots", f"kernel {plan.kernel} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, err=err, conv=conv,
                 its=its, werr=werr, wconv=wconv, wits=wits)
        if (launch.path == 0) != (max_iters == 0):
            fail("bpots", f"kernel {plan.kernel}: launch path {launch.path} {text}")
        done.add(plan.kernel)
        if launch.path != 0:             # max_iters == 0 launches no kernel: compared, but no tier has run
            ran["bpots"].add(plan.kernel)
            legs_run["bpots"] += 1


# ---- the leg of the fourth generator -----------------------------------------------------------------------------------
def decim_on_chip_width(H):
    """The tile width of the unforced plan (ldpc_debug_decim_tile_plan: host code, no device needed) where it is the on-chip
    tier, 0 where not even one syndrome fits.  Draws nothing."""
    import ctypes

    s, n = H.shape
    deg = np.diff(sp.csr_matrix(H).indptr)
    rec_words = int(np.where(deg == 0, 0, np.where(deg <= 32, 4, np.where(deg <= 64, 5, deg))).sum())
    tier, S = ctypes.c_int32(0), ctypes.c_int32(0)
    L = ldpc._capi.lib()
    ldpc._capi.check(L.ldpc_debug_decim_tile_plan(s, n, rec_words, 0, ctypes.byref(tier), ctypes.byref(S), None), L)
    return S.value if tier.value == 1 else 0


def leg_decim(H, B, run):
    """Guided-decimation min-sum on the case's graph against the numpy model: errors, flags, iteration and decimation counts
    and the LLR bit patterns.  Rounds of 0 ... 4 iterations and few decimations, or -- on a graph of at most 48 bits -- rounds
    of one iteration and every bit free to be pinned (the |D| == n exit), so that a leg stays within about 50 iterations."""
    g = rng4
    s, n = H.shape
    every_bit = g.random() < 0.3
    T, Dmax = int(g.choice([0, 1, 2, 4])), min(n, int(g.choice([0, 1, 3, 8])))
    if every_bit and n <= 48:
        T, Dmax = 1, n
    alpha, clip = float(g.choice([0.5, 0.75, 1.0])), float(g.choice([4.0, 20.0, 1e6]))
    prior = draw_priors(n, g)
    device_entry, want_decimated = bool(g.random() < 0.5), bool(g.random() < 0.5)
    Bd = min(B, 65)
    syn = draw_syndromes(H, Bd, g)
    text = (f"round_iters {T} max_decimations {Dmax} alpha {alpha} clip {clip} batch {Bd} {'device' if device_entry else 'host'} entry "
            f"decimated={want_decimated} n {n} S {decim_on_chip_width(H)}")
    if DRY or VERBOSE:
        print(f"   decim {text}", flush=True)
    if not run:
        return
    merr, mconv, mits, mdec, mL = timed_model("decim", lambda: DecimModel(H, prior, T, Dmax, alpha=alpha, clip=clip).decode(syn))
    if not GPU:
        return

    def go(dec, variant):
        if device_entry:
            err, conv = torch.full((Bd, n), 7, dtype=torch.uint8, device="cuda"), torch.full((Bd,), 7, dtype=torch.uint8, device="cuda")
            llr = torch.full((Bd, n), 7.0, dtype=torch.float64, device="cuda")
            its = torch.full((Bd,), -7, dtype=torch.int32, device="cuda")
            nd = torch.full((Bd,), -7, dtype=torch.int32, device="cuda") if want_decimated else None
            dec.decode_batch_device(dev(syn), err, conv, llr, its, nd)
            torch.cuda.synchronize()
            err, conv, llr, its = (x.cpu().numpy() for x in (err, conv, llr, its))
            nd = nd.cpu().numpy() if want_decimated else None
        else:
            out = dec.decode_batch_host(syn, want_llr=True, want_decimated=want_decimated)
            err, conv, llr, its = out[:4]
            nd = out[4] if want_decimated else None
        ok = same(err, merr) and same(conv, mconv) and same(its, mits) and same_bits(llr, mL) and (nd is None or same(nd, mdec))
        if not ok:
            fail("decim", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, prior=prior,
                 err=err, conv=conv, its=its, llr=llr, nd=nd, merr=merr, mconv=mconv, mits=mits, mdec=mdec, mL=mL)

    on_every_tier("decim", (1, 2), lambda v: ldpc.DecimatedMinSumDecoder(H, None, T, channel_llr=prior, max_decimations=Dmax, alpha=alpha,
                                                                         clip=clip, kernel_variant=v), go, text)


# ---- the leg of the fifth generator ------------------------------------------------------------------------------------
class PauliRelayPerLeg(ldpc.PauliRelayMinSumDecoder):
    """A PauliRelayMinSumDecoder with an iteration count of its own for every leg (ldpc_pauli_relay_create takes one per
    leg, the class's constructor gives leg 0 one count and all later legs another); the sides need not commute.  The decode
    methods are the class's."""

    def __init__(self, Hx, Hz, priors, gammas, leg_iters, stop_after, alpha, clip, kernel_variant):
        import ctypes

        from ldpcdecoders_jl_amd._host import _pattern_of, css_pattern

        Mx, Mz = _pattern_of(Hx), _pattern_of(Hz)
        self.sparse_Hx, self.sparse_Hz = Mx, Mz
        self.n, self.rows_x, self.rows_z, self.device = int(Mx.shape[1]), int(Mx.shape[0]), int(Mz.shape[0]), 0
        self.prior_x, self.prior_y, self.prior_z = (np.ascontiguousarray(priors[k], dtype=np.float32) for k in range(3))
        self.gammas = np.ascontiguousarray(gammas, dtype=np.float32)
        self.leg_iters = np.ascontiguousarray(leg_iters, dtype=np.int32)
        self.legs = int(self.leg_iters.size)
        assert self.gammas.shape == (self.legs, self.n)
        pat_x, pat_z = css_pattern(Mx), css_pattern(Mz)
        opts = ldpc._capi.PauliRelayOptions()
        opts.device, opts.alpha, opts.clip = 0, float(alpha), float(clip)
        opts.kernel_variant, opts.stop_after = int(kernel_variant), int(stop_after)
        L = ldpc._capi.lib_for(None)
        self._create(L, L.ldpc_pauli_relay_create, self.n, ctypes.byref(pat_x), ctypes.byref(pat_z), self.prior_x.ctypes.data,
                     self.prior_y.ctypes.data, self.prior_z.ctypes.data, self.legs, self.gammas.ctypes.data, self.leg_iters.ctypes.data,
                     ctypes.byref(opts))


def leg_pauli_relay(H, B, run):
    """The Pauli relay on Hx = the case's H and a second drawn Hz (the recipe of the pauli leg): 1 ... 4 legs of 0 ... 6
    iterations each (a leg of 0 is skipped wherever it stands), gammas in (-0.3, 0.9) per qubit and leg, stop_after 1 ... 3;
    with one triple for every qubit the weights tie, and a tie keeps the earlier solution."""
    g = rng5
    rx, n = H.shape
    A, Hz = draw_hz(n, g)
    rz = Hz.shape[0]
    legs = int(g.integers(1, 5))
    leg_iters = [int(x) for x in g.integers(0, 7, size=legs)]
    gammas = g.uniform(-0.3, 0.9, size=(legs, n)).astype(np.float32)
    stop_after = int(g.integers(1, 4))
    alpha, clip, _ = draw_rule(g)
    probs, uniform = draw_pauli_probs(n, g)
    device_entry, want_llr, want_iters, want_sol = (bool(g.random() < 0.5) for _ in range(4))
    Bp = min(B, 65)
    sampled = bool(g.random() < 0.6)
    if sampled:                               # the syndromes of sampled Pauli errors: sx = Hx ez, sz = Hz ex
        rate = g.uniform(0.01, 0.15)
        ex, ez = ((g.random((Bp, n)) < rate).astype(np.uint8) for _ in range(2))
        sx, sz = ldpc.codes.syndromes_of(H, ez), ldpc.codes.syndromes_of(Hz, ex)
    else:
        sx, sz = g.integers(0, 2, (Bp, rx)).astype(np.uint8), g.integers(0, 2, (Bp, rz)).astype(np.uint8)
    running = [k for k in range(legs) if leg_iters[k] > 0]
    text = (f"Hz ({rz}, {n}) B {Bp} leg_iters {leg_iters} stop_after {stop_after} negative_gammas {int((gammas[running] < 0).sum())} "
            f"alpha {alpha} clip {clip} {'device' if device_entry else 'host'} entry llr={want_llr} iters={want_iters} "
            f"solutions={want_sol} uniform={uniform} {'sampled' if sampled else 'arbitrary'} syndromes")
    if DRY or VERBOSE:
        print(f"   pauli_relay {text} {degrees_text(H, 'hx')} {degrees_text(Hz, 'hz')}", flush=True)
    if not run:
        return
    tables = pauli_priors(probs)
    mgx, mgz, mconv, mits, msol, mM = timed_model(
        "pauli_relay", lambda: PauliRelayModel(H, Hz, tables, gammas, leg_iters, alpha=alpha, clip=clip, stop_after=stop_after).decode(sx, sz))
    if not GPU:
        return

    def go(dec, variant):
        if device_entry:
            gx, conv, llr, its = device_outputs(Bp, n, 3, want_llr, want_iters)
            gz = torch.full((Bp, n), 7, dtype=torch.uint8, device="cuda")
            sol = torch.full((Bp,), -7, dtype=torch.int32, device="cuda") if want_sol else None
            dec.decode_batch_device(dev(sx), dev(sz), gx, gz, conv, llr, its, sol)
            torch.cuda.synchronize()
            gx, gz, conv, llr, its, sol = (host_of(x) for x in (gx, gz, conv, llr, its, sol))
        else:
            out = dec.decode_batch_host(sx, sz, want_llr=want_llr, want_solutions=want_sol)
            gx, gz, conv, llr, its = out[:5]
            sol = out[5] if want_sol else None
            if (llr is None) != (not want_llr) or len(out) != (6 if want_sol else 5):
                fail("pauli_relay", f"the host entry returns outputs it was not asked for, or none, kernel_variant {variant} {text}")
        ok = (same(gx, mgx) and same(gz, mgz) and same(conv, mconv) and (its is None or same(its, mits))
              and (sol is None or same(sol, msol)) and (llr is None or same_bits(llr, mM)))
        if not ok:
            fail("pauli_relay", f"kernel_variant {variant} {text}", hx_colptr=H.indptr, hx_rowval=H.indices, hx_shape=H.shape, hz=A,
                 probs=probs, gammas=gammas, leg_iters=leg_iters, sx=sx, sz=sz, gx=gx, gz=gz, conv=conv, its=its, sol=sol, llr=llr,
                 mgx=mgx, mgz=mgz, mconv=mconv, mits=mits, msol=msol, mM=mM)

    on_every_tier("pauli_relay", (1, 2), lambda v: PauliRelayPerLeg(H, Hz, tables, gammas, leg_iters, stop_after, alpha, clip, v), go, text)


# ---- the leg of the sixth generator ------------------------------------------------------------------------------------
OSD_SEARCH_BATCH_CAP = 65      # (the model is one dense elimination and up to 2080 candidates per syndrome)


def leg_osd_search(H, B, run):
    """The OSD step by the standard rule (ldpc_osd_set_search) on the case's graph against osd_search_model, per syndrome
    and in every element: both methods, the orders at their edges (0; 64 is clamped to K by the sweep), Hamming cost or
    weights -- drawn floats with negative entries, all zero (every candidate costs 0: the first wins), or values that clamp
    to +-2^40 --, a share of rows whose bp_err already reproduces the syndrome (step 1: the output is bp_err), LLRs with
    ties, +-0.0, +-inf and NaN.  Every syndrome is H e: none lies outside the column space."""
    g = rng6
    s, n = H.shape
    if g.random() < 0.6:
        method, order = "combination_sweep", int(g.choice([0, 1, 2, 10, 64]))
    else:
        method, order = "exhaustive", int(g.choice([0, 1, 3, 8]))
    kind = ("none", "floats", "zero", "clamped")[int(g.integers(0, 4))]
    weights = {"none": None, "floats": g.normal(1.0, 2.0, n), "zero": np.zeros(n),
               "clamped": g.choice([1e9, 2.0 ** 24, 1.0, 2.0 ** -16, -2.0 ** 24, -1e9], size=n)}[kind]
    inplace = bool(g.random() < 0.5)
    Bo = min(B, OSD_SEARCH_BATCH_CAP)
    E = (g.random((Bo, n)) < 0.1).astype(np.uint8)
    syn = ldpc.codes.syndromes_of(H, E)
    bp_err = (g.random((Bo, n)) < 0.1).astype(np.uint8)
    own = g.random(Bo) < 0.25                 # step 1: an estimate that reproduces the syndrome is returned unchanged
    bp_err[own] = E[own]
    reproducing = int((ldpc.codes.syndromes_of(H, bp_err) == syn).all(axis=1).sum())
    llr = g.normal(1.0, 3.0, (Bo, n))
    llr[g.random((Bo, n)) < 0.3] = llr[0, 0]        # ties
    llr[g.random((Bo, n)) < 0.05] = 0.0
    llr[g.random((Bo, n)) < 0.05] = -0.0
    if g.random() < 0.4:
        llr[g.random((Bo, n)) < 0.05] = np.nan
        llr[g.random((Bo, n)) < 0.03] = -np.inf
        llr[g.random((Bo, n)) < 0.03] = np.inf
    text = (f"{method} order {order} weights {kind} batch {Bo} reproducing_rows {reproducing} nan={bool(np.isnan(llr).any())} "
            f"{'in place' if inplace else 'out of place'}")
    if DRY or VERBOSE:
        print(f"   osd_search {text}", flush=True)
    if not run:
        return
    Hd = np.asarray(H.todense()).astype(np.uint8)
    q = None if weights is None else osd_search_weights_of(weights)
    want = timed_model("osd_search", lambda: np.stack([osd_search_model(Hd, syn[b], bp_err[b], llr[b], OSD_SEARCH_METHODS[method], order, q)
                                                       for b in range(Bo)]).astype(np.uint8))
    if not same(ldpc.codes.syndromes_of(H, want), syn):
        fail("osd_search", f"a model output does not reproduce its syndrome {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape,
             syn=syn, bp_err=bp_err, llr=llr, want=want)
    if not GPU:
        return

    class Post:
        def __init__(self, variant):
            self.post = ldpc.OSDPostProcessor(H, order, method=method, weights=weights)
            try:
                self.post.prepare_device(0, variant)
            except ldpc.LdpcError:
                self.post.close()
                raise
            self.kernel = self.post.kernel

        def close(self):
            self.post.close()

    def go(h, variant):
        d_err = dev(bp_err)
        out = h.post.postprocess_device(dev(syn), d_err, dev(llr), out=d_err if inplace else None)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if not same(got, want) or not (inplace or same(d_err.cpu().numpy(), bp_err)):
            fail("osd_search", f"kernel_variant {variant} {text}", colptr=H.indptr, rowval=H.indices, shape=H.shape, syn=syn, bp_err=bp_err,
                 llr=llr, weights=weights, got=got, want=want)

    on_every_tier("osd_search", (1, 2, 3), Post, go, text)


# ---- the leg of the seventh generator ----------------------------------------------------------------------------------
STAB_BATCH_CAP = 65      # (the model walks the union graph, which has more edges than the case's)


def draw_sz(s, n, g):
    """(A dense, Sz csc): a second pattern of the case's shape, sparser than the first, with an empty row and a row of
    33 ... 80 ones now and then; where it meets the case's pattern the edge is Y-type."""
    A = (g.random((s, n)) < g.uniform(0.01, 0.12)).astype(np.uint8)
    if g.random() < 0.35:
        A[g.integers(0, s), :] = 0
    if g.random() < 0.4 and n >= 33:          # a row of 33 ... 80 ones
        A[g.integers(0, s), g.choice(n, size=min(n, int(g.integers(33, 81))), replace=False)] = 1
    Sz = sp.csc_matrix(A)
    Sz.sort_indices()
    return A, Sz


def leg_stab(H, B, run):
    """The stabilizer min-sum on Sx = the case's H and a second drawn Sz of the same shape: an edge only H stores is X-type,
    one only Sz stores Z-type, one both store Y-type.  The rows need not commute (check=False)."""
    g = rng7
    r, n = H.shape
    A, Sz = draw_sz(r, n, g)
    alpha, clip, max_iters = draw_rule(g)
    probs, uniform = draw_pauli_probs(n, g)
    device_entry, want_llr, want_iters = (bool(g.random() < 0.5) for _ in range(3))
    Bs = min(B, STAB_BATCH_CAP)
    sampled = bool(g.random() < 0.6)
    if sampled:                               # the syndromes of sampled Pauli errors: s = Sx ez ^ Sz ex
        rate = g.uniform(0.01, 0.15)
        ex, ez = ((g.random((Bs, n)) < rate).astype(np.uint8) for _ in range(2))
        syn = ldpc.codes.syndromes_of(H, ez) ^ ldpc.codes.syndromes_of(Sz, ex)
    else:
        syn = g.integers(0, 2, (Bs, r)).astype(np.uint8)
    Hd = np.asarray(H.todense()) != 0
    union = sp.csc_matrix((Hd | (A != 0)).astype(np.uint8))
    text = (f"B {Bs} alpha {alpha} clip {clip} max_iters {max_iters} {'device' if device_entry else 'host'} entry llr={want_llr} "
            f"iters={want_iters} uniform={uniform} {'sampled' if sampled else 'arbitrary'} syndromes x_edges {int((Hd & (A == 0)).sum())} "
            f"z_edges {int((~Hd & (A != 0)).sum())} y_edges {int((Hd & (A != 0)).sum())}")
    if DRY or VERBOSE:
        print(f"   stab {text} {degrees_text(union, 'checks')}", flush=True)
    if not run:
        return
    tables = pauli_priors(probs)
    mgx, mgz, mconv, mits, mG = timed_model(
        "stab", lambda: StabMinSumModel(H, Sz, tables, max_iters, alpha=alpha, clip=clip).decode(syn))
    if not GPU:
        return

    def go(dec, variant):
        for name, got, want in zip("xyz", (dec.prior_x, dec.prior_y, dec.prior_z), tables):
            if not (got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))):
                fail("stab", f"prior_{name} differs from the model's table {text}", probs=probs, got=got, want=want)
        if device_entry:
            gx, conv, llr, its = device_outputs(Bs, n, 3, want_llr, want_iters)
            gz = torch.full((Bs, n), 7, dtype=torch.uint8, device="cuda")
            dec.decode_batch_device(dev(syn), gx, gz, conv, llr, its)
            torch.cuda.synchronize()
            gx, gz, conv, llr, its = (host_of(x) for x in (gx, gz, conv, llr, its))
        else:
            gx, gz, conv, llr, its = dec.decode_batch_host(syn, want_llr=want_llr)
            if (llr is None) != (not want_llr):
                fail("stab", f"the host entry returns LLRs it was not asked for, or none, kernel_variant {variant} {text}")
        ok = (same(gx, mgx) and same(gz, mgz) and same(conv, mconv) and (its is None or same(its, mits))
              and (llr is None or same_bits(llr, mG)))
        if not ok:
            fail("stab", f"kernel_variant {variant} {text}", sx_colptr=H.indptr, sx_rowval=H.indices, shape=H.shape, sz=A, probs=probs,
                 syn=syn, gx=gx, gz=gz, conv=conv, its=its, llr=llr, mgx=mgx, mgz=mgz, mconv=mconv, mits=mits, mG=mG)

    on_every_tier("stab", (1, 2), lambda v: ldpc.StabilizerMinSumDecoder(H, Sz, None, max_iters, pauli_probs=probs, alpha=alpha, clip=clip,
                                                                         kernel_variant=v, check=False), go, text)


# ---- the cases ---------------------------------------------------------------------------------------------------------
last_note = t0
for case in range(ncases):
    run = (not DRY) and FROM <= case <= TO
    kind, H = draw_graph()
    B = int(rng.choice([1, 2, 63, 64, 65, 130]))
    if DRY or VERBOSE:
        cdeg, bdeg = np.diff(sp.csr_matrix(H).indptr), np.diff(H.indptr)
        print(f"case {case}: kind {kind} shape {H.shape} nnz {H.nnz} B {B} checks<=32 {int(((cdeg > 0) & (cdeg <= 32)).sum())} "
              f"checks33-64 {int(((cdeg > 32) & (cdeg <= 64)).sum())} checks>64 {int((cdeg > 64).sum())} empty_checks {int((cdeg == 0).sum())} "
              f"empty_bits {int((bdeg == 0).sum())} max_bit_degree {int(bdeg.max())}", flush=True)
    leg_bitflip(H, B, run)
    leg_minsum(H, B, run)
    leg_relay(H, B, run)
    leg_osd(H, B, run)
    leg_trials(H, B, run)
    leg_css(B, run)
    leg_layered(H, B, run)
    leg_priors(H, B, run)
    leg_pauli(H, B, run)
    leg_bpots(H, B, run)
    leg_decim(H, B, run)
    leg_pauli_relay(H, B, run)
    leg_osd_search(H, B, run)
    leg_stab(H, B, run)
    if time.time() - last_note > 60:   # a silent GPU job looks hung to the runner
        last_note = time.time()
        print(f"... {case + 1} cases, {time.time() - t0:.0f} s", flush=True)

if MODEL_ONLY:
    print("model seconds: " + ", ".join(f"{c} {model_s[c]:.2f}" for c in TIERS), flush=True)
what = "drawn" if DRY else "through the models only" if MODEL_ONLY else "compared with the models on the GPU"
print(f"fuzz ok: {ncases} random cases {what} in {time.time() - t0:.0f} s (models {sum(model_s.values()):.0f} s), seed {seed}; "
      + "; ".join(f"{c} tiers {sorted(ran[c])} legs {legs_run[c]} skipped {skipped[c]}" for c in TIERS))
