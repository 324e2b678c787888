#!/usr/bin/env python
"""Times the min-sum entries with per-syndrome priors (ldpcdecoders.jl_amd/minsum.py: decode_batch_priors_device,
decode_batch_given_device) against the plain entry of the same handle, and the correlated CSS trials loop against the
uncorrelated one.

  python tools/priors_probe.py [--out profiles/priors_probe.txt] [--warmup 2] [--reps 7]

Cases (every one in a process of its own, started from here):
  (a) bb72, c1000, c16384 -- the graphs and batches of tools/layered_probe.py (BB-72 H_X at 0.06, batch 2^20, 30
      iterations; (1000,10,9) at 0.01, batch 2^18, 50 iterations; (16384,8,4) at 0.02, batch 2^16, 50 iterations), with both
      schedules.  Every priors row equals the handle's channel_llr and both tables of the given form equal it too, so the
      three entries run the same iterations on the same syndromes and must write the same bytes (checked); what differs is
      the staging of the priors, the P block of the flooding schedule and any change of S or tier it brings.  Measured
      against: the plain entry of the same handle.  Reported beside each time: the tier and S of the plan the entry ran.
  (b) css -- run_css_trials on BB-72, depolarizing 0.06, layered min-sum (30 iterations, per = 2 p / 3) on both sides,
      65,536 trials per call as one batch, correlated=True against correlated=False: time per call and the six counts.
Every time is a pair of device events around one call (for (b): a host clock around the call, which ends in the read-back
of the counts), after `warmup` untimed calls per entry; the entries are timed in turn, repetition by repetition, so that
all see the same machine; median and spread (max - min) over `reps`.  Nothing is tuned here and no ratio is asserted."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("bb72", "c1000", "c16384", "css")


def graph_of(ldpc, name):
    import scipy.sparse as sp

    if name == "bb72":
        return "BB-72 H_X", sp.csc_matrix(np.asarray(ldpc.codes.bivariate_bicycle_72_12_6()[0], dtype=np.uint8)), 0.06, 30, 1 << 20
    if name == "c1000":
        return "(1000,10,9)", ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 50, 1 << 18
    return "(16384,8,4)", ldpc.codes.parity_check_csc(16384, 8, 4), 0.02, 50, 1 << 16


def run_entries(name, warmup, reps):
    import torch

    import ldpcdecoders_jl_amd as ldpc

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    title, H, per, iters, B = graph_of(ldpc, name)
    n = H.shape[1]
    tr = ldpc.Trials(H)
    syn = tr.sample(B, per, seed=1)[1]
    torch.cuda.synchronize()
    tr.close()
    print(f"{title}, errors at {per}: batch {B}, max_iters {iters}; priors {B * n * 4 / 2**20:.0f} MiB as floats, {B * n / 2**20:.0f} MiB as given bits",
          flush=True)
    ok = True
    for schedule in ("flooding", "layered"):
        dec = ldpc.MinSumDecoder(H, per, iters, schedule=schedule)
        dec.set_conditional_priors(dec.channel_llr, dec.channel_llr)
        priors = torch.from_numpy(dec.channel_llr).cuda().repeat(B, 1).contiguous()
        given = (torch.arange(B * n, device="cuda", dtype=torch.int32).reshape(B, n) & 3).to(torch.uint8)
        outs = {k: (torch.empty((B, n), dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda"),
                    torch.empty(B, dtype=torch.int32, device="cuda")) for k in ("plain", "floats", "given")}
        calls = {"plain": lambda o: dec.decode_batch_device(syn, o[0], o[1], None, o[2]),
                 "floats": lambda o: dec.decode_batch_priors_device(syn, priors, o[0], o[1], None, o[2]),
                 "given": lambda o: dec.decode_batch_given_device(syn, given, o[0], o[1], None, o[2])}
        times = {k: [] for k in calls}
        for i in range(warmup + reps):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(outs[k])
                b.record()
                b.synchronize()
                if i >= warmup:
                    times[k].append(a.elapsed_time(b))
        info = dec.info()
        plan = {"plain": (info.kernel, info.tile_syndromes), "floats": (info.priors_kernel, info.priors_tile_syndromes),
                "given": (info.priors_kernel, info.priors_tile_syndromes)}
        its = outs["plain"][2]
        print(f"  {schedule}: mean iterations {float(its.float().mean()):.2f}, converged {float((outs['plain'][1] != 0).float().mean()) * 100:.2f} %",
              flush=True)
        base = float(np.median(times["plain"]))
        for k in calls:
            ts = np.array(times[k])
            same = all(bool(torch.equal(x, y)) for x, y in zip(outs[k], outs["plain"]))
            ok = ok and same
            print(f"    {k:6s} tier {plan[k][0]}, S {plan[k][1]:2d}: median {np.median(ts):9.3f} ms, spread {ts.max() - ts.min():7.3f} ms;"
                  f" {np.median(ts) / base:5.2f} x plain; equals the plain entry's output: {'yes' if same else 'NO'}", flush=True)
        dec.close()
        del priors, given, outs
    return ok


def run_css(warmup, reps):
    import scipy.sparse as sp

    import ldpcdecoders_jl_amd as ldpc

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    Hx, Hz = (sp.csc_matrix(np.asarray(M, dtype=np.uint8)) for M in ldpc.codes.bivariate_bicycle_72_12_6())
    p, B = 0.06, 65536
    dx = ldpc.MinSumDecoder(Hx, 2 * p / 3, 30, schedule="layered")
    dz = ldpc.MinSumDecoder(Hz, 2 * p / 3, 30, schedule="layered")
    times, res = {False: [], True: []}, {}
    for i in range(warmup + reps):
        for correlated in (False, True):
            t0 = time.perf_counter()
            res[correlated] = ldpc.run_css_trials(dx, dz, B, p, batch=B, seed=1, correlated=correlated)
            if i >= warmup:
                times[correlated].append(time.perf_counter() - t0)
    print(f"BB-72, depolarizing {p}, layered min-sum on both sides (30 iterations, per 2 p / 3), one batch of {B} per call", flush=True)
    for correlated in (False, True):
        ts, r = np.array(times[correlated]) * 1e3, res[correlated]
        print(f"  correlated={correlated!s:5s}: median {np.median(ts):8.3f} ms per batch, spread {ts.max() - ts.min():7.3f} ms; counts: trials {r.trials},"
              f" block {r.block_errors}, syndrome mismatch {r.syndrome_mismatches}, logical {r.logical_errors}, logical X {r.logical_x_errors},"
              f" logical Z {r.logical_z_errors}; not converged hx {r.not_converged_hx}, hz {r.not_converged_hz}", flush=True)
    dx.close()
    dz.close()
    return res[True].logical_x_errors == res[False].logical_x_errors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priors_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--case", choices=CASES, help="run this case here (what the probe starts once per case)")
    args = ap.parse_args()
    assert args.reps >= 1 and args.warmup >= 1
    if args.case:
        ok = run_css(args.warmup, args.reps) if args.case == "css" else run_entries(args.case, args.warmup, args.reps)
        sys.exit(0 if ok else 1)
    lines = [f"priors_probe: one box, a process per case, {args.reps} repetitions after {args.warmup} warm-up(s) per entry, the entries in turn;"
             " (a) time = device events around one device-entry call, measured against the plain entry of the same handle on the same"
             " syndromes (every priors row = channel_llr: same iterations); (b) time = host clock around one run_css_trials call of one"
             " batch, correlated against uncorrelated; spread = max - min"]
    print(lines[0], flush=True)
    all_ok = True
    for name in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--warmup", str(args.warmup), "--reps", str(args.reps)],
                             capture_output=True, text=True, timeout=900)
        text = out.stdout.rstrip("\n")
        print(text, flush=True)
        lines.append(text)
        if out.returncode != 0:
            all_ok = False
            lines.append(f"  case {name} FAILED (exit code {out.returncode}): {out.stderr.strip()[-400:]}")
            print(lines[-1], flush=True)
            break                                  # nothing more is started on a device a case has failed on
    lines.append(f"all cases: {'ok' if all_ok else 'FAILED'}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all_ok, "a case failed (see above)"


if __name__ == "__main__":
    main()
