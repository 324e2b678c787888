#!/usr/bin/env python
"""Times the Pauli relay min-sum decoder against the decoders it joins, on the same trials, and scores every decoder's
guesses.  Nothing here is a pass criterion: the numbers are measured, not tuned.

  python tools/pauli_relay_probe.py [--out profiles/pauli_relay_probe.txt] [--reps 5]

Code: BB-72 under depolarizing noise of total rate 0.03, 0.06 and 0.09; batch 65,536 each.  Decoders:
    Pauli relay               PauliRelayMinSumDecoder at its defaults (9 legs of 30, 20, ... iterations, stop_after = 1)
    Pauli relay, stop 3       the same with stop_after = 3
    Pauli min-sum(30)         PauliMinSumDecoder(30)
    two relay sides           RelayMinSumDecoder at its defaults on Hz (for the X parts) and on Hx (for the Z parts), each at
                              the marginal rate 2 p / 3, as run_css_trials drives them

Every case runs in a process of its own, under its own `timeout -k 10` (this script starts itself once per case, one at a
time), and the first case that fails ends the run: nothing more starts on a device that has just failed a case.  The
trials are the same in all of them: CSSTrials.sample(batch, p, seed=1) on the device, a rule that depends on nothing but
its arguments.  Time: a host clock around the device-entry call (the two calls of the two sides) that ends in a device
synchronise, after one untimed call; median and spread (max - min) over `reps`.  Share converged: the decoder's flags
(both sides' for the two relay sides).  Logical failure rate: run_css_joint_trials / run_css_trials over the same trials
(same seed, same sampling rule).  Iterations: mean and maximum over the batch (per side for the two relay sides).  The
maximum is what holds a tile: a workgroup's tile ends with its slowest lane.  No threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ldpcdecoders_jl_amd as ldpc  # noqa: E402

BATCH = 1 << 16
RATES = (0.03, 0.06, 0.09)
CASES = ("prelay", "prelay3", "pauli", "sides")
NAMES = {"prelay": "Pauli relay (defaults)", "prelay3": "Pauli relay, stop_after 3", "pauli": "Pauli min-sum(30)",
         "sides": "two relay sides (defaults)"}


def run_case(p, case, reps):
    import torch

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    dev = torch.device("cuda", 0)
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    Hx, Hz = sp.csc_matrix(np.asarray(Hx) != 0), sp.csc_matrix(np.asarray(Hz) != 0)
    n, B = 72, BATCH
    tr = ldpc.CSSTrials(Hx, Hz)
    ex, ez, sx, sz = tr.sample(B, p, seed=1)
    tr.close()
    gx, gz = (torch.empty((B, n), dtype=torch.uint8, device=dev) for _ in range(2))
    conv, conv2 = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(2))
    its, its2 = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    if case in ("prelay", "prelay3"):
        dec = ldpc.PauliRelayMinSumDecoder(Hx, Hz, p, stop_after=3 if case == "prelay3" else 1)
        decs = (dec,)

        def call():
            dec.decode_batch_device(sx, sz, gx, gz, conv, None, its)
    elif case == "pauli":
        dec = ldpc.PauliMinSumDecoder(Hx, Hz, p, 30)
        decs = (dec,)

        def call():
            dec.decode_batch_device(sx, sz, gx, gz, conv, None, its)
    else:
        dec_hz, dec_hx = ldpc.RelayMinSumDecoder(Hz, 2.0 * p / 3.0, 30), ldpc.RelayMinSumDecoder(Hx, 2.0 * p / 3.0, 30)
        decs = (dec_hx, dec_hz)

        def call():
            dec_hz.decode_batch_device(sz, gx, conv, None, its)       # Hz sees the X parts
            dec_hx.decode_batch_device(sx, gz, conv2, None, its2)

    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ok = conv if case != "sides" else conv & conv2
    res = dict(p=p, case=case, batch=B, median_ms=float(np.median(ts)) * 1e3, spread_ms=float(max(ts) - min(ts)) * 1e3,
               converged=float((ok != 0).float().mean()), mean_iters=float(its.float().mean()), max_iters=int(its.max()),
               tier=int(decs[0].kernel), tile_syndromes=int(decs[0].info().tile_syndromes), device=torch.cuda.get_device_name(0))
    if case == "sides":
        res["mean_iters2"], res["max_iters2"] = float(its2.float().mean()), int(its2.max())
        r = ldpc.run_css_trials(dec_hx, dec_hz, B, p, batch=B, seed=1)
    else:
        r = ldpc.run_css_joint_trials(dec, B, p, batch=B, seed=1)
    res.update(logical_errors=r.logical_errors, logical_x_errors=r.logical_x_errors, logical_z_errors=r.logical_z_errors,
               syndrome_mismatches=r.syndrome_mismatches, block_errors=r.block_errors)
    for d in decs:
        d.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_relay_probe.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", nargs=2, metavar=("P", "DECODER"), help="run one case in this process (internal)")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    args = ap.parse_args()
    assert args.reps >= 5
    if args.case:
        return run_case(float(args.case[0]), args.case[1], args.reps)
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    first = True
    try:
        for p in RATES:
            for case in CASES:
                q = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                                    "--case", str(p), case], capture_output=True, text=True)
                got = [x for x in q.stdout.splitlines() if x.startswith("RESULT ")]
                if q.returncode != 0 or not got:   # nothing more runs on a device that has just failed a case
                    say(f"BB-72, p {p}, {NAMES[case]}: FAILED (exit {q.returncode})\n{q.stderr[-2000:]}")
                    raise SystemExit(1)
                r = json.loads(got[-1][7:])
                if first:
                    say(f"pauli_relay_probe: {r['device']}, one box, {args.reps} repetitions after 1 warm-up, every case in a process of its own;"
                        " time = host clock around the device-entry call(s) + device synchronise; spread = max - min")
                    first = False
                if case == CASES[0]:
                    say(f"BB-72 (36 + 36 checks x 72 qubits), depolarizing p {p}, batch {r['batch']}:")
                B = r["batch"]
                iters = f"iterations mean {r['mean_iters']:7.3f} max {r['max_iters']}"
                if "mean_iters2" in r:
                    iters = f"iterations Hz side mean {r['mean_iters']:7.3f} max {r['max_iters']}, Hx side mean {r['mean_iters2']:7.3f} max {r['max_iters2']}"
                say(f"  {NAMES[case]:28s} tier {r['tier']} S {r['tile_syndromes']:2d}  median {r['median_ms']:9.3f} ms, spread {r['spread_ms']:7.3f} ms;"
                    f" converged {r['converged'] * 100:7.3f} %; logical failure rate {r['logical_errors'] / B:.3e} ({r['logical_errors']} of {B}:"
                    f" {r['logical_x_errors']} X, {r['logical_z_errors']} Z; {r['syndrome_mismatches']} miss a syndrome); {iters}")
    finally:   # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
