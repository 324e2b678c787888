#!/usr/bin/env python
"""Times the guided-decimation min-sum decoder against the library's other answers to stalled min-sum, on the same
syndromes, and scores every decoder's guesses.  Nothing here is a pass criterion: the numbers are measured, not tuned.

  python tools/decim_probe.py [--out profiles/decim_probe.txt] [--reps 5]

Codes: BB-72 H_X at 0.03 and 0.06, and (16384, 8, 4) at 0.02; batch 65,536 each.  Decoders:
    decimation, Dmax n   DecimatedMinSumDecoder, 10 iterations a round, every bit may be pinned
    decimation, Dmax 8   DecimatedMinSumDecoder, 10 iterations a round, at most 8 decimations
    min-sum              MinSumDecoder(30)
    relay                RelayMinSumDecoder at its defaults
    min-sum + OSD-0      BeliefPropagationOSDDecoder(osd="device", osd_order=0, bp_decoder=MinSumDecoder(30)); BB-72 only
On (16384, 8, 4) a syndrome that never converges holds its tile for 10 * (Dmax + 1) iterations, 163,850 with Dmax = n: that
case runs only if the Dmax = 8 case before it converged everywhere, and is reported as not run otherwise.

Every case runs in a process of its own, under its own `timeout -k 10` (this script starts itself once per case, one at a
time), and the first case that fails ends the run: nothing more starts on a device that has just failed a case.  The
syndromes are the same in all of them: Trials.sample(batch, per, seed=1) on the device, a rule that depends on nothing
but its arguments.  Time: a host clock around one device-entry call that ends in a device synchronise, after one untimed
call; median and spread (max - min) over `reps`.  Share converged: the decoder's flags.  Logical failure rate (BB-72):
run_trials(decoder, batch, per, seed=1, logicals=Lz) -- block errors: the guess misses the syndrome or differs from the
error by a logical operator; on (16384, 8, 4), without logicals, guess != error.  No threshold."""
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
CODES = {"bb72": ("BB-72 H_X", (0.03, 0.06)), "big": ("(16384,8,4)", (0.02,))}
QLDPC_CASES = ("decim_n", "decim_8", "minsum", "relay", "osd0")
BIG_CASES = ("decim_8", "decim_n", "minsum", "relay")
NAMES = {"decim_n": "decimation, 10 a round, Dmax n", "decim_8": "decimation, 10 a round, Dmax 8", "minsum": "min-sum(30)",
         "relay": "relay (defaults)", "osd0": "min-sum(30) + OSD-0 (device)"}


def code_of(key):
    """-> (H, logicals or None)"""
    if key == "big":
        return ldpc.codes.parity_check_csc(16384, 8, 4), None
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    return sp.csc_matrix(np.asarray(sp.csc_matrix(Hx).todense(), dtype=np.uint8)), Lz


def run_case(key, per, case, reps):
    import torch

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    dev = torch.device("cuda", 0)
    H, Lz = code_of(key)
    s, n = H.shape
    B = BATCH
    tr = ldpc.Trials(H, Lz)
    e, syn = tr.sample(B, per, seed=1)
    err = torch.empty((B, n), dtype=torch.uint8, device=dev)
    conv = torch.empty(B, dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    ndec = torch.empty(B, dtype=torch.int32, device=dev)
    inner = None
    if case in ("decim_n", "decim_8"):
        dec = ldpc.DecimatedMinSumDecoder(H, per, 10, max_decimations=None if case == "decim_n" else 8)
    elif case == "relay":
        dec = ldpc.RelayMinSumDecoder(H, per, 30)
    else:
        dec = inner = ldpc.MinSumDecoder(H, per, 30)
        if case == "osd0":
            dec = ldpc.BeliefPropagationOSDDecoder(H, osd_order=0, osd="device", bp_decoder=inner)
    out = {}

    def call():
        if case == "osd0":
            out["guess"], out["conv"], _ = dec.batchdecode_device(syn)
        elif case in ("decim_n", "decim_8"):
            dec.decode_batch_device(syn, err, conv, None, its, ndec)
            out["guess"], out["conv"] = err, conv
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
               unconverged=int((out["conv"] == 0).sum()), block_errors=int(c[1]), syndrome_mismatches=int(c[2]),
               tier=int((inner or dec).kernel), device=torch.cuda.get_device_name(0))
    if case != "osd0":   # (the OSD wrapper does not hand the iteration counts on)
        res["mean_iters"], res["max_iters"] = float(its.float().mean()), int(its.max())
    if case in ("decim_n", "decim_8"):
        res["mean_decimated"], res["max_decimated"] = float(ndec.float().mean()), int(ndec.max())
    tr.close()
    if Lz is not None:   # the logical failure rate, through the trials loop: the same sampling rule, so the same syndromes
        r = ldpc.run_trials(dec, B, per=per, batch=B, seed=1, logicals=Lz)
        res["trials_block_errors"], res["trials_logical_errors"], res["trials_not_converged"] = r.block_errors, r.logical_errors, r.not_converged
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decim_probe.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", nargs=3, metavar=("CODE", "PER", "DECODER"), help="run one case in this process (internal)")
    ap.add_argument("--limit", type=int, default=180, help="seconds a case may take")
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
        for key, (title, pers) in CODES.items():
            cases = BIG_CASES if key == "big" else QLDPC_CASES
            for per in pers:
                everywhere = True   # big: did the Dmax = 8 case converge on every syndrome?
                for case in cases:
                    if key == "big" and case == "decim_n" and not everywhere:
                        say(f"  {NAMES[case]:32s} not run: the unconverged syndromes above would each hold a tile for up to 163,850 iterations")
                        continue
                    p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                                        "--case", key, str(per), case], capture_output=True, text=True)
                    got = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
                    if p.returncode != 0 or not got:   # nothing more runs on a device that has just failed a case
                        say(f"{title}, per {per}, {NAMES[case]}: FAILED (exit {p.returncode})\n{p.stderr[-2000:]}")
                        raise SystemExit(1)
                    r = json.loads(got[-1][7:])
                    if first:
                        say(f"decim_probe: {r['device']}, one box, {args.reps} repetitions after 1 warm-up, every case in a process of its own;"
                            " time = host clock around one device-entry call + device synchronise; spread = max - min")
                        first = False
                    if case == cases[0]:
                        say(f"{title} ({r['s']} x {r['n']}), per {per}, batch {r['batch']}:")
                    if case == "decim_8":
                        everywhere = r["unconverged"] == 0
                    B = r["batch"]
                    more = f"; iterations mean {r['mean_iters']:7.2f} max {r['max_iters']}" if "mean_iters" in r else ""
                    if "mean_decimated" in r:
                        more += f"; decimations mean {r['mean_decimated']:6.3f} max {r['max_decimated']}"
                    if "trials_block_errors" in r:
                        fail = (f"logical failure rate {r['trials_block_errors'] / B:.3e} ({r['trials_block_errors']} of {B} through run_trials;"
                                f" {r['syndrome_mismatches']} miss the syndrome)")
                    else:
                        fail = f"guess != error {r['block_errors'] / B:.3e} ({r['block_errors']} of {B}; {r['syndrome_mismatches']} miss the syndrome)"
                    say(f"  {NAMES[case]:32s} tier {r['tier']}  median {r['median_ms']:10.3f} ms, spread {r['spread_ms']:8.3f} ms;"
                        f" converged {r['converged'] * 100:7.3f} %; {fail}{more}")
    finally:   # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
