#!/usr/bin/env python
"""Times the min-sum decoder's device entry (ldpcdecoders.jl_amd/minsum.py) and checks what it timed.

  python tools/minsum_probe.py [--out profiles/minsum_probe.txt] [--warmup 2] [--reps 5]

Shapes: BB-72 H_X, batch 2^20 (per 0.03, 30 iterations); parity_check_matrix(1000, 10, 9), batch 2^18 (per 0.01, 50);
(16384, 8, 4), batch 65,536 at per 0.02 (50), and the same on uniformly random syndromes, which neither decoder matches:
every column runs all 50 iterations.  The syndromes come from Trials.sample on the device.  BeliefPropagationDecoder --
existing code, the yardstick -- is timed in the same process on the same syndromes with the same iteration limit; the
mean iteration count of each decoder is printed next to its time, because the two rules stop at different iterations.
Every time is a host clock around one call that ends in a device synchronise, after `warmup` untimed calls; median and
spread (max - min) over `reps`.

For the unlimited tier the probe prints the bytes its lanes request per iteration by this traffic model (4-byte words
per syndrome; deg <= 32 everywhere at these shapes):
    check sweep   nnz (L of every edge) + 4 s (record read) + 4 s (record written), + s bytes of syndrome
    bit sweep     3 nnz (a, one magnitude, one sign word per edge) + n (L written)   (channel_llr is shared by all lanes)
summed over the sweeps every column ran (iters + 1 check sweeps: the last one carries the stop test), over the median
time, as a fraction of the 8 TB/s HBM peak.  It is requested traffic: what the caches serve never reaches HBM, so the
figure is an upper bound of the HBM share, not a measurement of it.

The only gate: on a sample of 4,096 syndromes in all (2,048 / 1,024 / 768 / 256 over the four runs) errors, flags,
iteration counts and LLR bit patterns equal the numpy model (tests/minsum_model.py).  No speed threshold."""
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
from minsum_model import MinSumModel, llr_of_probs  # noqa: E402

HBM_PEAK = 8.0e12


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minsum_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 1
    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    dev = torch.device("cuda", 0)
    say(f"minsum_probe: {torch.cuda.get_device_name(0)}, one box, {args.reps} repetitions after {args.warmup} warm-ups; "
        "time = host clock around one device-entry call + device synchronise; spread = max - min")
    bb = sp.csc_matrix(np.asarray(ldpc.codes.bivariate_bicycle_72_12_6()[0], dtype=np.uint8))
    big = ldpc.codes.parity_check_csc(16384, 8, 4)
    runs = [("BB-72 H_X", bb, 0.03, 30, 1 << 20, False, 2048),
            ("(1000,10,9)", ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 50, 1 << 18, False, 1024),
            ("(16384,8,4)", big, 0.02, 50, 1 << 16, False, 768),
            ("(16384,8,4), random syndromes (forced 50 iterations)", big, 0.02, 50, 1 << 16, True, 256)]
    gate_ok = True
    for name, H, per, max_iters, B, forced, nsample in runs:
        s, n = H.shape
        nnz = int(H.nnz)
        tr = ldpc.Trials(H)
        _, syn = tr.sample(B, per, seed=1)
        if forced:
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            syn = torch.randint(0, 2, (B, s), dtype=torch.uint8, device=dev, generator=g)
        tr.close()
        err = torch.empty((B, n), dtype=torch.uint8, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        its = torch.empty(B, dtype=torch.int32, device=dev)
        ms = ldpc.MinSumDecoder(H, per, max_iters)
        ms_med, ms_spread = timed(lambda: ms.decode_batch_device(syn, err, conv, None, its), torch, args.warmup, args.reps)
        ms_its = its.cpu().numpy().astype(np.int64)
        ms_conv = float(conv.float().mean())
        say(f"{name}: batch {B}, per {per}, max_iters {max_iters}; min-sum tier {ms.kernel}")
        say(f"  min-sum      median {ms_med * 1e3:9.3f} ms, spread {ms_spread * 1e3:8.3f} ms; mean iterations {ms_its.mean():6.2f},"
            f" converged {ms_conv * 100:6.2f} %  -> {B / ms_med / 1e6:8.3f} M syndromes/s")
        if ms.kernel == 2:
            check_b, bit_b = 4 * (nnz + 8 * s) + s, 4 * (3 * nnz + n)
            total = float(((ms_its + 1) * check_b + ms_its * bit_b).sum())
            say(f"  traffic model: {check_b + bit_b} bytes requested per syndrome and iteration ({check_b} check sweep + {bit_b} bit sweep);"
                f" {total / 1e9:.1f} GB over the call -> {total / ms_med / 1e12:.3f} TB/s requested = {total / ms_med / HBM_PEAK * 100:.1f} %"
                " of the 8 TB/s HBM peak (an upper bound of the HBM share: cache hits are counted)")
        # the gate: a sample of columns against the model
        idx = np.unique(np.linspace(0, B - 1, nsample).astype(np.int64))
        llr = torch.empty((len(idx), n), dtype=torch.float64, device=dev)
        sub = syn[torch.from_numpy(idx).to(dev)].contiguous()
        e2, c2, i2 = err[: len(idx)].clone(), conv[: len(idx)].clone(), its[: len(idx)].clone()
        ms.decode_batch_device(sub, e2, c2, llr, i2)
        torch.cuda.synchronize()
        full = (err.cpu().numpy()[idx], conv.cpu().numpy()[idx], ms_its[idx])
        t0 = time.perf_counter()
        say(f"  model on {len(idx)} columns ...")
        merr, mconv, mits, mL = MinSumModel(H, llr_of_probs(np.full(n, per)), max_iters).decode(sub.cpu().numpy())
        ok = (np.array_equal(e2.cpu().numpy(), merr) and np.array_equal(c2.cpu().numpy(), mconv)
              and np.array_equal(i2.cpu().numpy(), mits)
              and np.array_equal(llr.cpu().numpy().view(np.int64), mL.astype(np.float64).view(np.int64))
              and np.array_equal(full[0], merr) and np.array_equal(full[1], mconv) and np.array_equal(full[2], mits))
        gate_ok &= ok
        say(f"  sample of {len(idx)} columns equal to the model (errors, flags, iterations, LLR bits; in the timed batch and alone):"
            f" {'yes' if ok else 'NO'}  ({time.perf_counter() - t0:.0f} s of model)")
        ms.close()
        # the yardstick: existing code, same syndromes, same iteration limit
        bp = ldpc.BeliefPropagationDecoder(H, per, max_iters, device=0)
        bp_med, bp_spread = timed(lambda: bp.decode_batch_device(syn, err, conv, None, its), torch, args.warmup, args.reps)
        say(f"  sum-product  median {bp_med * 1e3:9.3f} ms, spread {bp_spread * 1e3:8.3f} ms; mean iterations {float(its.float().mean()):6.2f},"
            f" converged {float(conv.float().mean()) * 100:6.2f} %  (kernel {bp.info().last_kernel})")
        say(f"  min-sum / sum-product time: {ms_med / bp_med:.2f} x")
        bp.close()
        del err, conv, its, syn, llr, sub
        torch.cuda.empty_cache()
    say(f"gate (outputs equal the model on the samples): {'pass' if gate_ok else 'FAIL'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert gate_ok, "the gate failed (see above)"


if __name__ == "__main__":
    main()
