#!/usr/bin/env python
"""Times the sliding-window step and sliding-window decoding (ldpcdecoders.jl_amd/windows.py) and checks what it timed.

  python tools/window_probe.py [--out profiles/window_probe.txt] [--warmup 1] [--reps 5] [--batch 65536]

1. The step kernel alone -- the commit of window 0 of the phenomenological BB-72 H_X model at R = 6, W = 3, C = 1, with
   the fused gather of window 1 -- against a device-to-device copy of the same byte count (bytes read + bytes written by
   the step: the window's guess, |commit_0| guess bytes, |U_0| residual bytes both ways, the next window's syndromes) in
   the same run, in turn.  The ratio of the medians says how far the glue is from a plain copy; no bound is set here.
2. SlidingWindowDecoder (W = 3, C = 1) around MinSumDecoder (30 iterations, channel_probs) against one MinSumDecoder of
   the whole model, at R = 6, 12 and 24, on the same `sample_rates` syndromes: time, tile width S and tier of each
   handle, the share of converged columns and the logical failure rate through `Trials.score`.
Every time is a host clock around one call that ends in a device synchronise, after `warmup` untimed calls; median and
spread (max - min) over `reps`.  The first 32 columns of every timed sliding-window decode are compared with the CPU
model chain (tests/windows_model.py around tests/minsum_model.py).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P_DATA, Q_MEAS, WIDTH, COMMIT, ITERS = 0.01, 0.02, 3, 1, 30


def median_spread(ts):
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.max() - ts.min())


def timed(fn, args, torch):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median_spread(ts)


def step_case(ldpc, torch, args, say):
    import windows_model as wm

    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    dem = ldpc.phenomenological(HX, ldpc.codes.css_logicals(HX, HZ)[1], 6, P_DATA, Q_MEAS)
    plan = ldpc.window_plan(dem, ldpc.phenomenological_layers(HX, 6), WIDTH, COMMIT)
    w = plan.windows
    step = ldpc.WindowStep(dem.H, [x.det for x in w], [x.mech for x in w], [x.commit for x in w])
    B = args.batch
    gen = torch.Generator(device="cuda").manual_seed(1)
    wg = torch.randint(0, 2, (B, w[0].mech.size), dtype=torch.uint8, device="cuda", generator=gen)
    res0 = torch.randint(0, 2, (B, dem.num_detectors), dtype=torch.uint8, device="cuda", generator=gen)
    res = res0.clone()
    guess = torch.zeros((B, dem.num_mechanisms), dtype=torch.uint8, device="cuda")
    nxt = torch.empty((B, w[1].det.size), dtype=torch.uint8, device="cuda")
    cols = wm._columns(dem.H)
    owned = {d for c in w[0].commit for d in cols[int(w[0].mech[c])]} | set(w[1].det.tolist())
    moved = B * (w[0].mech.size + w[0].commit.size + 2 * len(owned) + w[1].det.size)
    half = moved // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    ts, tc = [], []
    for i in range(args.warmup + args.reps):                       # in turn, so that both see the same machine
        for fn, acc in ((lambda: step.commit(0, wg, res, guess, next_syndromes=nxt), ts), (lambda: dst.copy_(src), tc)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                acc.append(time.perf_counter() - t0)
    (s_med, s_spread), (c_med, c_spread) = median_spread(ts), median_spread(tc)
    # what it timed: one commit from the untouched residual against the model, 32 columns
    res.copy_(res0)
    step.commit(0, wg, res, guess, next_syndromes=nxt)
    n = min(B, 32)
    m_res, m_guess = res0[:n].cpu().numpy().copy(), np.zeros((n, dem.num_mechanisms), dtype=np.uint8)
    windows = [dict(det=x.det, mech=x.mech, commit=x.commit) for x in w]
    m_next = wm.commit(dem.H, windows, 0, wg[:n].cpu().numpy(), m_res, m_guess, want_next=True)
    ok = (np.array_equal(res[:n].cpu().numpy(), m_res) and np.array_equal(guess[:n].cpu().numpy(), m_guess)
          and np.array_equal(nxt[:n].cpu().numpy(), m_next))
    say(f"step kernel, phenomenological BB-72 H_X R = 6, commit of window 0 + gather of window 1, batch {B}:"
        f" guess column {w[0].mech.size} B, {w[0].commit.size} committed, |U_0| = {len(owned)}, next {w[1].det.size}")
    say(f"  step: median {s_med * 1e3:.3f} ms, spread {s_spread * 1e3:.3f} ms -> {moved / s_med / 1e12:.3f} TB/s moved")
    say(f"  copy of {half} B (the same bytes read + written): median {c_med * 1e3:.3f} ms, spread {c_spread * 1e3:.3f} ms"
        f" -> the step takes {s_med / c_med:.2f} x the copy; equal to the model in {n} columns: {'yes' if ok else 'NO'}")
    step.close()
    return ok


def decode_case(ldpc, torch, args, say, R):
    import windows_model as wm
    from minsum_model import MinSumModel, llr_of_probs

    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    dem = ldpc.phenomenological(HX, ldpc.codes.css_logicals(HX, HZ)[1], R, P_DATA, Q_MEAS)
    layers = ldpc.phenomenological_layers(HX, R)
    B = args.batch
    make = lambda m: ldpc.MinSumDecoder(m.H, None, ITERS, channel_probs=m.rates)   # noqa: E731
    tr = dem.trials()
    err, syn = tr.sample_rates(B, seed=1)
    say(f"phenomenological BB-72 H_X, R = {R}: {dem.num_mechanisms} mechanisms, {dem.num_detectors} detectors, batch {B}")
    ok = True
    for name, dec in (("one-shot min-sum", make(dem)), (f"sliding window W = {WIDTH}, C = {COMMIT}", ldpc.SlidingWindowDecoder(dem, layers, WIDTH, COMMIT, make))):
        guess = torch.empty((B, dem.num_mechanisms), dtype=torch.uint8, device="cuda")
        conv = torch.empty(B, dtype=torch.uint8, device="cuda")
        med, spread = timed(lambda: dec.decode_batch_device(syn, guess, conv), args, torch)
        _, counts = tr.score(guess, err, want_flags=False)
        c = counts.cpu().tolist()
        handles = dec.decoders if hasattr(dec, "decoders") else [dec]
        shape = ", ".join(f"S {h.info().tile_syndromes} tier {h.info().kernel}" for h in handles)
        say(f"  {name}: median {med * 1e3:.3f} ms, spread {spread * 1e3:.3f} ms; handles: {shape}; converged"
            f" {float((conv != 0).float().mean()):.5f}; logical failure rate {c[3] / c[0]:.3e} ({c[3]} of {c[0]})")
        if hasattr(dec, "plan"):
            n = min(B, 32)
            windows, uncovered = wm.plan(dem.H, layers, WIDTH, COMMIT)

            def decode_of(H, rates):
                model = MinSumModel(H, llr_of_probs(rates), ITERS)
                return lambda s: model.decode(s)[:2]
            want = wm.chain(dem.H, dem.rates, windows, uncovered, decode_of, syn[:n].cpu().numpy())
            ok = np.array_equal(guess[:n].cpu().numpy(), want[0]) and np.array_equal(conv[:n].cpu().numpy(), want[1])
            say(f"    equal to the model chain in {n} columns: {'yes' if ok else 'NO'}")
        dec.close()
    tr.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_probe.txt"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1 << 16)
    args = ap.parse_args()
    import torch

    import ldpcdecoders_jl_amd as ldpc

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)
    say(f"window_probe on {torch.cuda.get_device_name(0)}: one box, one process, {args.reps} repetitions after {args.warmup} warm-up(s);"
        " time = host clock around one call + device synchronise; spread = max - min")
    all_ok = step_case(ldpc, torch, args, say)
    for R in (6, 12, 24):
        all_ok = decode_case(ldpc, torch, args, say, R) and all_ok
    say(f"all cases: {'ok' if all_ok else 'FAILED'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all_ok, "a case differs from the model (see above)"


if __name__ == "__main__":
    main()
