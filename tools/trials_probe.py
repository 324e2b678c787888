#!/usr/bin/env python
"""Times the Monte-Carlo trial steps (ldpcdecoders.jl_amd/trials.py) and checks what it timed.

  python tools/trials_probe.py [--out profiles/trials_probe.txt] [--warmup 2] [--reps 5]

1. Trials.sample (errors + syndromes, one kernel) against the torch formulation the benchmark uses for the same job
   (`make_syndromes`, imported from the unmodified bench.py), at three shapes: (16384, 8, 4) batch 65,536; BB-72 H_X
   batch 2^20; parity_check_matrix(1000, 10, 9) batch 2^18.  The gate: the new entry's median is below the torch
   one by more than the two spreads (max - min) together, at every shape.  Bytes/s = batch * (n + s) written / time.
2. Trials.score at the same shapes (guesses = the errors with a seeded flip in every third column): ms and bytes/s
   (2 * batch * n read).
3. run_trials at n 16384, per 0.02, 50 BP iterations, 2^20 trials in batches of 65,536: wall time per batch and the share
   that is sample + score.
Every time is a host clock around one call that ends in a device synchronise, after `warmup` untimed calls; median and
spread over `reps`.  A column sample of every timed output is compared with the CPU model (tests/trials_model.py).
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ldpcdecoders_jl_amd as ldpc  # noqa: E402
import trials_model as tm  # noqa: E402
from bench import make_syndromes  # noqa: E402


def timed(fn, torch, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.max() - ts.min())


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trials_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=1 << 20)
    args = ap.parse_args()
    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    dev = torch.device("cuda", 0)
    say(f"trials_probe: {torch.cuda.get_device_name(0)}, one box, {args.reps} repetitions after {args.warmup} warm-ups; "
        "time = host clock around one call + device synchronise; spread = max - min")
    big = ldpc.codes.parity_check_csc(16384, 8, 4)
    shapes = [("(16384,8,4)", big, 0.02, 1 << 16),
              ("BB-72 H_X", sp.csc_matrix(ldpc.codes.bivariate_bicycle_72_12_6()[0]), 0.02, 1 << 20),
              ("(1000,10,9)", ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 1 << 18)]
    say("note: the two sides are not like for like.  make_syndromes returns the syndromes only (its errors are dropped chunk by"
        " chunk) and uploads the graph's index arrays in every call; Trials.sample writes errors AND syndromes.  The ratio is the"
        " new entry against what the parent offers for the job, and the TB/s line counts the new entry's bytes alone.")
    gate_ok = True
    for name, H, per, B in shapes:
        s, n = H.shape
        Hcsr = sp.csr_matrix(H)
        Hcsr.sort_indices()
        t = ldpc.Trials(H)
        err = torch.empty((B, n), dtype=torch.uint8, device=dev)
        syn = torch.empty((B, s), dtype=torch.uint8, device=dev)
        new_med, new_spread = timed(lambda: t.sample(B, per, seed=1, out=(err, syn)), torch, args.warmup, args.reps)
        old_med, old_spread = timed(lambda: make_syndromes(torch, Hcsr, n, B, per, 1, dev), torch, args.warmup, args.reps)
        idx = np.unique(np.linspace(0, B - 1, 48).astype(np.int64))
        h_err, h_syn = err[idx].cpu().numpy(), syn[idx].cpu().numpy()
        want = np.concatenate([tm.sample(n, 1, per, 1, int(i)) for i in idx])
        ok = np.array_equal(h_err, want) and np.array_equal(h_syn, tm.syndromes(H, want))
        passed = new_med + new_spread + old_spread < old_med
        gate_ok &= passed and ok
        say(f"{name} batch {B} per {per}, tier {t.kernel}")
        say(f"  sample (errors + syndromes): median {new_med * 1e3:.3f} ms, spread {new_spread * 1e3:.3f} ms"
            f"  -> {B * (n + s) / new_med / 1e12:.3f} TB/s written (conversion kernels of profiles/bit_io_kernel_stats.csv: 4.8 TB/s)")
        say(f"  torch make_syndromes (bench.py): median {old_med * 1e3:.3f} ms, spread {old_spread * 1e3:.3f} ms"
            f"  -> {old_med / new_med:.1f} x; gate (median below by more than both spreads): {'pass' if passed else 'FAIL'};"
            f" sample of {len(idx)} columns equal to the model: {'yes' if ok else 'NO'}")
        guess = err.clone()
        guess[::3, n // 2] ^= 1
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        flags = torch.empty(B, dtype=torch.uint8, device=dev)
        sc_med, sc_spread = timed(lambda: t.score(guess, err, flags=flags, counts=counts), torch, args.warmup, args.reps)
        calls = args.warmup + args.reps
        want_counts = [B * calls, calls * len(range(0, B, 3))]
        ok = counts.cpu().tolist()[:2] == want_counts and bool((flags[::3] & 1).all()) and not bool(flags[1::3].any())
        gate_ok &= ok
        say(f"  score: median {sc_med * 1e3:.3f} ms, spread {sc_spread * 1e3:.3f} ms -> {2 * B * n / sc_med / 1e12:.3f} TB/s read;"
            f" counts after {calls} calls as expected: {'yes' if ok else 'NO'}")
        t.close()
        del err, syn, guess, flags
        torch.cuda.empty_cache()

    # 3. the whole loop at the headline shape
    per, B = 0.02, 1 << 16
    dec = ldpc.BeliefPropagationDecoder(big, per, 50, device=0)
    res = [None]

    def loop():
        res[0] = ldpc.run_trials(dec, args.trials, batch=B, seed=1)

    run_med, run_spread = timed(loop, torch, args.warmup, args.reps)
    nb = (args.trials + B - 1) // B
    t = ldpc.Trials(big)
    err = torch.empty((B, 16384), dtype=torch.uint8, device=dev)
    syn = torch.empty((B, 8192), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)

    def sample_and_score():
        t.sample(B, per, seed=1, out=(err, syn))
        t.score(err, err, counts=counts, want_flags=False)

    ss_med, ss_spread = timed(sample_and_score, torch, args.warmup, args.reps)
    say(f"run_trials (16384,8,4) per {per}, 50 iterations, {args.trials} trials in {nb} batches of {B}: median {run_med * 1e3:.1f} ms,"
        f" spread {run_spread * 1e3:.1f} ms -> {run_med / nb * 1e3:.2f} ms per batch (decode step of BENCH_r04: 47.6 ms)")
    say(f"  sample + score of one batch alone: median {ss_med * 1e3:.3f} ms, spread {ss_spread * 1e3:.3f} ms"
        f" -> {ss_med / (run_med / nb) * 100:.1f} % of a batch;  result: {res[0]}")
    t.close()
    dec.close()
    say(f"gate: {'pass' if gate_ok else 'FAIL'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert gate_ok, "the gate failed (see above)"


if __name__ == "__main__":
    main()
