#!/usr/bin/env python
"""Times BitFlipDecoder.decode_batch_device and checks what it timed.

  python tools/bitflip_probe.py [--reps 7] [--sample 64] > profiles/bitflip_probe.txt

Configurations: the reference's (parity_check_matrix(1000, 10, 9), per 0.01, 100 iterations; tier 1) at batch 1, 4,096
and 2^20, and one graph per tier: (16384, 8, 4) on tier 2, and the reference's graph forced through tiers 2 and 3.
Each timing is a host clock around `reps` back-to-back calls' worth of single calls that end in a device synchronise
(after one warm-up call); the minimum, the median and the spread (max - min over the median) are printed.  The outputs
of the last timed call are compared with the CPU model (tests/bitflip_model.py) on an evenly spaced sample of columns, and
the model's own time on ONE CPU core for that sample, scaled to the batch, is printed next to it: the honest yardstick
where the reference cannot run (no Julia here).  No speed is promised anywhere; this is a measurement.
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
from bitflip_model import TIE_RANDOM, BitFlipModel  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=64)
    args = ap.parse_args()
    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    small = ldpc.codes.parity_check_csc(1000, 10, 9)
    large = ldpc.codes.parity_check_csc(16384, 8, 4)
    configs = [
        # (name, H, per, max_iters, kernel_variant, batch)
        ("reference (1000,10,9) tier 1", small, 0.01, 100, 0, 1),
        ("reference (1000,10,9) tier 1", small, 0.01, 100, 0, 4096),
        ("reference (1000,10,9) tier 1", small, 0.01, 100, 0, 1 << 20),
        ("(16384,8,4) tier 2", large, 0.002, 100, 0, 4096),
        ("reference (1000,10,9) forced tier 2", small, 0.01, 100, 2, 4096),
        ("reference (1000,10,9) forced tier 3", small, 0.01, 100, 3, 4096),
    ]
    print(f"bitflip_probe: {torch.cuda.get_device_name(0)}, reps {args.reps} (+1 warm-up), sample {args.sample} columns vs the model")
    print("time per call = host clock around one decode_batch_device call + device synchronise; spread = (max - min) / median")
    for name, H, per, max_iters, variant, B in configs:
        n = H.shape[1]
        chunk = 1 << 16
        syn = np.concatenate([ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, min(chunk, B - a), per, seed=1000 + a))
                              for a in range(0, B, chunk)])
        dec = ldpc.BitFlipDecoder(H, per, max_iters, seed=1, kernel_variant=variant)
        d_syn = torch.from_numpy(syn).cuda()
        err = torch.empty((B, n), dtype=torch.uint8, device="cuda")
        conv = torch.empty((B,), dtype=torch.uint8, device="cuda")
        its = torch.empty((B,), dtype=torch.int32, device="cuda")
        stop = torch.empty((B,), dtype=torch.uint8, device="cuda")
        times = []
        for r in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_batch_device(d_syn, err, conv, its, stop, column0=0)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        times = np.array(times[1:])
        h_err, h_conv, h_its, h_stop = err.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy(), stop.cpu().numpy()
        idx = np.unique(np.linspace(0, B - 1, min(args.sample, B)).astype(np.int64))
        model = BitFlipModel(H, max_iters)
        t0 = time.process_time()
        ok = True
        for i in idx:
            w = model.decode_batch(syn[i:i + 1], TIE_RANDOM, seed=1, column0=int(i))
            ok &= bool(np.array_equal(w[0][0], h_err[i]) and w[1][0] == h_conv[i] and w[2][0] == h_its[i] and w[3][0] == h_stop[i])
        model_s = (time.process_time() - t0) / len(idx) * B
        total_iters = int(h_its.astype(np.int64).sum())
        med = float(np.median(times))
        print(f"{name}: tier {dec.kernel}, batch {B}, iterations {total_iters} (mean {total_iters / B:.1f}), "
              f"stop reasons {np.bincount(h_stop, minlength=3).tolist()}")
        print(f"    GPU per call: min {times.min() * 1e3:.3f} ms, median {med * 1e3:.3f} ms, spread {(times.max() - times.min()) / med * 100:.1f} %"
              f"  -> {B / med:.0f} syndromes/s, {med / max(total_iters, 1) * 1e9:.1f} ns per iteration (batch-wide)")
        print(f"    model, one CPU core, scaled from {len(idx)} columns: {model_s * 1e3:.1f} ms per batch;"
              f" sample equal to the model: {'yes' if ok else 'NO'}")
        assert ok, "timed output differs from the model"
        dec.close()
        del d_syn, err, conv, its, stop


if __name__ == "__main__":
    main()
