#!/usr/bin/env python3
"""Throughput of the HOST-buffer entries (what a Julia batchdecode! call hits: host arrays in, host arrays out, PCIe
included) next to the HBM-resident entries: the byte entry (one byte per bit), the bits entry (Julia BitMatrix layout,
ldpc_bp_decode_batch_bits) and the two device entries, for the small-code workloads and the headline case.

The entries of a case run ALTERNATING (byte host, bits host, byte device, bits device, and again), `--reps` timed
rounds after `--warmup` untimed ones; medians and min-max are printed, and the byte entry's own spread is the noise floor
for the ratios.  `--kernel-stats CSV` turns the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of this
script into the conversion kernels' times and achieved GB/s."""
import argparse
import csv
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "bb72": ("BB-72 per=0.005", lambda ldpc: sp.csc_matrix(ldpc.codes.bivariate_bicycle_72_12_6()[0]), 0.005, 1 << 20),
    "n1008": ("(3,6) n=1008 per=0.01", lambda ldpc: ldpc.codes.parity_check_csc(1008, 6, 3), 0.01, 1 << 18),
    "n16384": ("(4,8) n=16384 per=0.02", lambda ldpc: ldpc.codes.parity_check_csc(16384, 8, 4), 0.02, 1 << 14),
    "headline": ("headline n=16384 (8,4) per=0.02", lambda ldpc: ldpc.codes.parity_check_csc(16384, 8, 4), 0.02, 1 << 16),
}


def stats(ts):
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def run_case(ldpc, torch, key, reps, warmup, entries):
    name, make, per, B = CASES[key]
    H = make(ldpc)
    H.sort_indices()
    s, n = H.shape
    base = min(B, 1 << 12 if key == "headline" else 1 << 16)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, base, per, seed=1))
    syn = np.ascontiguousarray(np.tile(syn, (B // syn.shape[0], 1)))
    dec = ldpc.BeliefPropagationDecoder(H, per, 50)
    out = (np.empty((B, n), dtype=np.uint8), np.empty(B, dtype=np.uint8))   # caller-owned, reused
    syn_bm = ldpc.BitMatrix.from_dense(syn.T)                               # s x B, packed once outside the timing
    err_bm = ldpc.BitMatrix.zeros(n, B)
    d_syn = torch.from_numpy(syn).cuda()
    d_err = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_conv = torch.empty(B, dtype=torch.uint8, device="cuda")
    d_syn_w = torch.from_numpy(syn_bm.chunks.view(np.int64)).cuda()
    d_err_w = torch.zeros(err_bm.chunks.size, dtype=torch.int64, device="cuda")

    def host_byte():
        t0 = time.perf_counter(); dec.decode_batch_host(syn, out=out); return (time.perf_counter() - t0) * 1e3

    def host_bits():
        t0 = time.perf_counter(); dec.decode_batch_bits_host(syn_bm, out=err_bm); return (time.perf_counter() - t0) * 1e3

    def dev_byte():
        dec.decode_batch_device(d_syn, d_err, d_conv); return dec.last_timing()[1]          # total_ms: HIP events

    def dev_bits():
        dec.decode_batch_bits_device(B, d_syn_w, 0, d_err_w, 0, d_conv); return dec.last_timing()[1]

    fns = {"host_byte": host_byte, "host_bits": host_bits, "dev_byte": dev_byte, "dev_bits": dev_bits}
    fns = {k: f for k, f in fns.items() if k in entries}
    times = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, f in fns.items():                                            # alternating
            t = f()
            if r >= warmup:
                times[k].append(t)
    if "host_byte" in fns and "host_bits" in fns:
        assert np.array_equal(err_bm.to_dense().T, out[0]), "the bits entry and the byte entry disagree"
    print(f"{name}  B={B}  s={s} n={n}  50 iterations  ({reps} timed repetitions after {warmup} warm-up, alternating)")
    med = {}
    for k, ts in times.items():
        m, lo, hi = stats(ts)
        med[k] = m
        print(f"    {k:10s} median {m:9.3f} ms   min {lo:9.3f}   max {hi:9.3f}   ({B / m / 1e3:8.2f} M syndromes/s)")
    if "host_byte" in med and "host_bits" in med:
        print(f"    host bits / host byte   {med['host_bits'] / med['host_byte']:.3f}")
    if "host_bits" in med and "dev_byte" in med:
        print(f"    host bits / device byte {med['host_bits'] / med['dev_byte']:.3f}")
    if "dev_bits" in med and "dev_byte" in med:
        _, lo, hi = stats(times["dev_byte"])
        diff = med["dev_bits"] - med["dev_byte"]
        inside = "inside" if abs(diff) <= hi - lo else "outside"
        print(f"    device bits / device byte {med['dev_bits'] / med['dev_byte']:.3f}   (difference {diff:+.3f} ms, "
              f"{inside} the byte entry's spread of {hi - lo:.3f} ms)")
    dec.close()


def kernel_stats(path, B, s, n):
    """Rows of the two conversion kernels out of rocprofv3's kernel statistics; bytes moved per call = count * (1 + 1/8)."""
    rows = list(csv.DictReader(open(path)))
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "calls", "total_ns", "average_ns", "bytes_per_call", "achieved_GB_per_s", "share_of_8_TB_per_s_peak"])
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        count = B * s if "bits_to_bytes" in name else B * n if "bytes_to_bits" in name else 0
        if not count:
            continue
        avg = float(r.get("AverageNs") or r.get("Average") or 0)
        moved = count * (1 + 1 / 8)
        gbs = moved / avg if avg else 0.0
        w.writerow([name, r.get("Calls"), r.get("TotalDurationNs") or r.get("TotalDuration"), f"{avg:.0f}", f"{moved:.0f}",
                    f"{gbs:.1f}", f"{gbs / 8000:.3f}"])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cases", default="bb72,n1008,n16384,headline")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--entries", default="host_byte,host_bits,dev_byte,dev_bits")
    ap.add_argument("--kernel-stats", help="kernel statistics CSV of a rocprofv3 run over ONE case: print the conversion kernels' rows")
    a = ap.parse_args()
    if a.kernel_stats:
        _, make, _, B = CASES[a.cases.split(",")[0]]
        import ldpcdecoders_jl_amd as ldpc
        s, n = make(ldpc).shape
        return kernel_stats(a.kernel_stats, B, s, n)
    import torch
    import ldpcdecoders_jl_amd as ldpc
    for key in a.cases.split(","):
        run_case(ldpc, torch, key, a.reps, a.warmup, a.entries.split(","))


if __name__ == "__main__":
    main()
