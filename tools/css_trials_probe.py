#!/usr/bin/env python
"""Times the CSS-code Monte-Carlo trial steps (ldpcdecoders.jl_amd/css_trials.py) and checks what it timed.

  python tools/css_trials_probe.py [--out profiles/css_trials_probe.txt] [--warmup 2] [--reps 7]

Two shapes: BB-72 at batch 2^20 (one wave per column) and the hypergraph product of parity_check_matrix(60, 6, 3)
(n = 4500, a workgroup per column) at batch 2^16, depolarizing p = 0.03.  At each shape, median and spread (max - min)
over `reps` repetitions after `warmup` untimed calls of
  1. CSSTrials.sample   (ex, ez, sx, sz in one kernel: one mix per qubit);
  2. CSSTrials.score    (guesses = the errors with a seeded flip in every third column);
  3. the yardstick: what two one-matrix handles do for the same job, minus the X/Z correlation -- Trials(Hz).sample and
     Trials(Hx).sample at per = 2p/3 (two mixes per qubit), and Trials(Hz).score plus Trials(Hx).score.
What to expect, not to assume: the fused sample should not be slower than the yardstick's by more than both spreads; the
report says whether that held.  Every time is a host clock around the calls and a device synchronise.  A column sample of
every timed output is compared with the CPU model (tests/css_trials_model.py).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ldpcdecoders_jl_amd as ldpc  # noqa: E402
import css_trials_model as cm  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "css_trials_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    dev = torch.device("cuda", 0)
    say(f"css_trials_probe: {torch.cuda.get_device_name(0)}, one box, {args.reps} repetitions after {args.warmup} warm-ups; "
        "time = host clock around the calls + device synchronise; spread = max - min")
    p = 0.03
    shapes = [("BB-72", ldpc.codes.bivariate_bicycle_72_12_6(), 1 << 20),
              ("HGP(60,6,3) n=4500", ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(60, 6, 3)), 1 << 16)]
    all_ok = True
    for name, (Hx, Hz), B in shapes:
        Lx, Lz = ldpc.codes.css_logicals(Hx, Hz)
        n, rx, rz = Hx.shape[1], Hx.shape[0], Hz.shape[0]
        t = ldpc.CSSTrials(Hx, Hz, logicals=(Lx, Lz))
        ex, ez = (torch.empty((B, n), dtype=torch.uint8, device=dev) for _ in range(2))
        sx = torch.empty((B, rx), dtype=torch.uint8, device=dev)
        sz = torch.empty((B, rz), dtype=torch.uint8, device=dev)
        new_med, new_spread = timed(lambda: t.sample(B, p, seed=1, out=(ex, ez, sx, sz)), torch, args.warmup, args.reps)
        idx = np.unique(np.linspace(0, B - 1, 48).astype(np.int64))
        want = [np.concatenate(a) for a in zip(*(cm.sample(n, 1, p, 1, int(i)) for i in idx))]
        want_sx, want_sz = cm.syndromes(Hx, Hz, want[0], want[1])
        ok = all(np.array_equal(got[idx].cpu().numpy(), w) for got, w in ((ex, want[0]), (ez, want[1]), (sx, want_sx), (sz, want_sz)))
        # the yardstick: two one-matrix handles (the X side through Hz, the Z side through Hx), no correlation
        tz, tx = ldpc.Trials(Hz, logicals=Lz), ldpc.Trials(Hx, logicals=Lx)
        e2, s2 = torch.empty_like(ex), torch.empty_like(sx)

        def two_samples():
            tz.sample(B, 2 * p / 3, seed=1, out=(ex, sz))
            tx.sample(B, 2 * p / 3, seed=2, out=(e2, s2))

        old_med, old_spread = timed(two_samples, torch, args.warmup, args.reps)
        held = new_med <= old_med + new_spread + old_spread
        all_ok &= ok
        say(f"{name} batch {B} p {p} (depolarizing), tier {t.kernel}, k = {Lx.shape[0]} logical qubits")
        say(f"  CSSTrials.sample (ex, ez, sx, sz): median {new_med * 1e3:.3f} ms, spread {new_spread * 1e3:.3f} ms"
            f"  -> {B * (2 * n + rx + rz) / new_med / 1e12:.3f} TB/s written; sample of {len(idx)} columns equal to the model: {'yes' if ok else 'NO'}")
        say(f"  yardstick, two Trials.sample: median {old_med * 1e3:.3f} ms, spread {old_spread * 1e3:.3f} ms"
            f"  -> fused / yardstick = {new_med / old_med:.2f}; not slower by more than both spreads: {'held' if held else 'DID NOT HOLD'}")
        t.sample(B, p, seed=1, out=(ex, ez, sx, sz))
        gx, gz = ex.clone(), ez.clone()
        gx[::3, n // 2] ^= 1
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        flags = torch.empty(B, dtype=torch.uint8, device=dev)
        sc_med, sc_spread = timed(lambda: t.score(gx, gz, ex, ez, flags=flags, counts=counts), torch, args.warmup, args.reps)
        calls = args.warmup + args.reps
        ok = counts.cpu().tolist()[:2] == [B * calls, calls * len(range(0, B, 3))] and bool((flags[::3] & 1).all()) and not bool(flags[1::3].any())
        all_ok &= ok
        c4 = torch.zeros(4, dtype=torch.int64, device=dev)

        def two_scores():
            tz.score(gx, ex, counts=c4, want_flags=False)
            tx.score(gz, ez, counts=c4, want_flags=False)

        ys_med, ys_spread = timed(two_scores, torch, args.warmup, args.reps)
        say(f"  CSSTrials.score: median {sc_med * 1e3:.3f} ms, spread {sc_spread * 1e3:.3f} ms -> {4 * B * n / sc_med / 1e12:.3f} TB/s read;"
            f" counts after {calls} calls as expected: {'yes' if ok else 'NO'}")
        say(f"  yardstick, two Trials.score (no flags): median {ys_med * 1e3:.3f} ms, spread {ys_spread * 1e3:.3f} ms"
            f"  -> fused / yardstick = {sc_med / ys_med:.2f}")
        for h in (t, tz, tx):
            h.close()
        del ex, ez, sx, sz, e2, s2, gx, gz, flags
        torch.cuda.empty_cache()
    say(f"outputs as the model says: {'yes' if all_ok else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all_ok, "a timed output differs from the model (see above)"


if __name__ == "__main__":
    main()
