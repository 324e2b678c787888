#!/usr/bin/env python
"""Times the relay min-sum decoder against what the library had before it, on the same syndromes, and scores every
decoder's guesses.

  python tools/relay_probe.py [--out profiles/relay_probe.txt] [--reps 5]

Codes: BB-72 H_X (2^20 syndromes) and H_X of hypergraph_product(parity_check_matrix(12, 4, 3)) (225 qubits, 2^16
syndromes), each at two error rates.  Decoders:
    relay            RelayMinSumDecoder at its defaults (9 legs of 30 / 20 iterations, stop_after 1)
    relay, gamma 0   RelayMinSumDecoder with gamma = 0 and one leg of 30: the work of MinSumDecoder(30), so the difference
                     is the cost of the second row (M next to X), the second pass over the messages and the bookkeeping
    min-sum          MinSumDecoder(30), existing code
    min-sum + OSD-0 / OSD-3   BeliefPropagationOSDDecoder(osd="device", bp_decoder=MinSumDecoder(30)), existing code
and (16384, 8, 4) at per 0.02, batch 65,536, where both decoders take the unlimited tier: relay at the defaults, relay
with gamma 0 and one leg of 50, and MinSumDecoder(50).

Every case runs in a process of its own (this script starts itself once per case, one at a time).  The syndromes are the
same in all of them: Trials.sample(batch, per, seed=1) on the device, a rule that depends on nothing but its arguments.
Time: a host clock around one device-entry call that ends in a device synchronise, after one untimed call; median and
spread (max - min) over `reps`.  Share converged: the decoder's flags.  Logical failure rate: Trials.score on those
guesses (block errors: the guess misses the syndrome or differs from the error by a logical operator).  No threshold."""
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

CODES = {"bb72": ("BB-72 H_X", 1 << 20, (0.03, 0.06)), "hgp225": ("HGP-225 H_X", 1 << 16, (0.01, 0.03)),
         "big": ("(16384,8,4)", 1 << 16, (0.02,))}
QLDPC_CASES = ("relay", "relay0", "minsum", "osd0", "osd3")
BIG_CASES = ("relay", "relay0", "minsum")
NAMES = {"relay": "relay (defaults)", "relay0": "relay, gamma 0, one leg", "minsum": "min-sum",
         "osd0": "min-sum + OSD-0 (device)", "osd3": "min-sum + OSD-3 (device)"}


def code_of(key):
    """-> (H, logicals or None)"""
    if key == "big":
        return ldpc.codes.parity_check_csc(16384, 8, 4), None
    if key == "bb72":
        Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    else:
        Hx, Hz = ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(12, 4, 3))
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    return sp.csc_matrix(np.asarray(sp.csc_matrix(Hx).todense(), dtype=np.uint8)), Lz


def run_case(key, per, case, reps):
    import torch

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    dev = torch.device("cuda", 0)
    H, Lz = code_of(key)
    s, n = H.shape
    B = CODES[key][1]
    iters0 = 50 if key == "big" else 30
    tr = ldpc.Trials(H, Lz)
    e, syn = tr.sample(B, per, seed=1)
    err = torch.empty((B, n), dtype=torch.uint8, device=dev)
    conv = torch.empty(B, dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    inner = None
    if case == "relay":
        dec = ldpc.RelayMinSumDecoder(H, per, iters0)
    elif case == "relay0":
        dec = ldpc.RelayMinSumDecoder(H, per, iters0, legs=1, gammas=np.zeros((1, n), dtype=np.float32))
    else:
        dec = inner = ldpc.MinSumDecoder(H, per, iters0)
        if case != "minsum":
            dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=int(case[3:]), osd="device", bp_decoder=inner)
    out = {}

    def call():
        if inner is not None and dec is not inner:
            out["guess"], out["conv"], _ = dec.batchdecode_device(syn)
        else:
            dec.decode_batch_device(syn, err, conv, None, its)
            out["guess"], out["conv"] = err, conv

    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tr.score(out["guess"], e, counts=counts, want_flags=False)
    c = counts.cpu().tolist()
    res = dict(code=key, per=per, case=case, batch=B, s=s, n=n, median_ms=float(np.median(ts)) * 1e3,
               spread_ms=float(max(ts) - min(ts)) * 1e3, converged=float(out["conv"].float().mean()),
               block_errors=int(c[1]), syndrome_mismatches=int(c[2]), logical_errors=int(c[3]),
               tier=int((inner or dec).kernel), device=torch.cuda.get_device_name(0))
    if case in BIG_CASES:   # (the OSD wrapper does not hand the iteration counts on)
        res["mean_iters"] = float(its.float().mean())
    tr.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relay_probe.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", nargs=3, metavar=("CODE", "PER", "DECODER"), help="run one case in this process (internal)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
    args = ap.parse_args()
    assert args.reps >= 5
    if args.case:
        return run_case(args.case[0], float(args.case[1]), args.case[2], args.reps)
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    first = True
    try:
        for key, (title, B, pers) in CODES.items():
            cases = BIG_CASES if key == "big" else QLDPC_CASES
            for per in pers:
                for case in cases:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--case", key, str(per), case],
                                       capture_output=True, text=True, timeout=args.limit)
                    got = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
                    if p.returncode != 0 or not got:   # nothing more runs on a device that has just failed a case
                        say(f"{title}, per {per}, {NAMES[case]}: FAILED (exit {p.returncode})\n{p.stderr[-2000:]}")
                        raise SystemExit(1)
                    r = json.loads(got[-1][7:])
                    if first:
                        say(f"relay_probe: {r['device']}, one box, {args.reps} repetitions after 1 warm-up, every case in a process of its own;"
                            " time = host clock around one device-entry call + device synchronise; spread = max - min")
                        first = False
                    if case == cases[0]:
                        say(f"{title} ({r['s']} x {r['n']}), per {per}, batch {B}:")
                    its = f"; mean iterations {r['mean_iters']:7.2f}" if "mean_iters" in r else ""
                    what = "logical failure rate" if key != "big" else "guess != error"
                    say(f"  {NAMES[case]:26s} tier {r['tier']}  median {r['median_ms']:10.3f} ms, spread {r['spread_ms']:8.3f} ms; converged {r['converged'] * 100:7.3f} %;"
                        f" {what} {r['block_errors'] / B:.3e} ({r['block_errors']} of {B}; {r['syndrome_mismatches']} miss the syndrome){its}")
    finally:   # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
