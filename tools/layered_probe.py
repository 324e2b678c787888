#!/usr/bin/env python
"""Times the two schedules of the min-sum decoder -- flooding and layered (ldpcdecoders.jl_amd/minsum.py, schedule=) -- on
the same syndromes and reports what each needed to converge.

  python tools/layered_probe.py [--out profiles/layered_probe.txt] [--warmup 1] [--reps 5]

Cases (every one in a process of its own, started from here):
  bb72      BB-72 H_X, errors at 0.06, batch 2^20, 30 iterations
  c1000     parity_check_matrix(1000, 10, 9), errors at 0.01, batch 2^18, 50 iterations
  c16384    (16384, 8, 4), errors at 0.02, batch 2^16, 50 iterations (the unlimited tier)
  dem6      the phenomenological BB-72 H_X model of tools/window_probe.py (p 0.01, q 0.02) at R = 6, one decoder over the
            whole model, batch 2^16, 30 iterations, per-bit priors from the rates
The syndromes come from Trials.sample (dem6: sample_rates) on the device, once per case; both decoders read the same
tensor.  Every time is a host clock around one device-entry call that ends in a device synchronise, after `warmup`
untimed calls per decoder; the two decoders are timed in turn, repetition by repetition, so that both see the same
machine; median and spread (max - min) over `reps`.  Reported per schedule: time, mean iteration count, share of
converged columns, the time per mean iteration, and K.  Where the graph is small enough for the numpy models
(n <= 2000), the first 32 columns of both decodes are compared with them (tests/minsum_model.py, tests/layered_model.py).
Nothing is tuned here and no speed is asserted."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("bb72", "c1000", "c16384", "dem6")
P_DATA, Q_MEAS = 0.01, 0.02


def case_inputs(ldpc, name):
    """-> (title, H, Trials, sampler() -> syndromes, constructor keywords, max_iters, batch)."""
    import scipy.sparse as sp

    if name == "dem6":
        HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
        dem = ldpc.phenomenological(HX, ldpc.codes.css_logicals(HX, HZ)[1], 6, P_DATA, Q_MEAS)
        tr = dem.trials()
        B = 1 << 16
        return (f"phenomenological BB-72 H_X, R = 6 ({dem.num_mechanisms} mechanisms, {dem.num_detectors} detectors)", dem.H, tr,
                lambda: tr.sample_rates(B, seed=1)[1], dict(per=None, channel_probs=dem.rates), 30, B)
    if name == "bb72":
        title, H = "BB-72 H_X", sp.csc_matrix(np.asarray(ldpc.codes.bivariate_bicycle_72_12_6()[0], dtype=np.uint8))
        per, iters, B = 0.06, 30, 1 << 20
    elif name == "c1000":
        title, H, per, iters, B = "(1000,10,9)", ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 50, 1 << 18
    else:
        title, H, per, iters, B = "(16384,8,4)", ldpc.codes.parity_check_csc(16384, 8, 4), 0.02, 50, 1 << 16
    tr = ldpc.Trials(H)
    return f"{title}, errors at {per}", H, tr, lambda: tr.sample(B, per, seed=1)[1], dict(per=per), iters, B


def run_case(name, warmup, reps):
    import torch

    import ldpcdecoders_jl_amd as ldpc

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    title, H, tr, sampler, kw, iters, B = case_inputs(ldpc, name)
    syn = sampler()
    torch.cuda.synchronize()
    tr.close()
    n = H.shape[1]
    per = kw.pop("per")
    decs, outs, times = {}, {}, {"flooding": [], "layered": []}
    for schedule in ("flooding", "layered"):
        decs[schedule] = ldpc.MinSumDecoder(H, per, iters, schedule=schedule, **kw)
        outs[schedule] = (torch.empty((B, n), dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda"),
                          torch.empty(B, dtype=torch.int32, device="cuda"))
    for i in range(warmup + reps):
        for schedule, dec in decs.items():
            err, conv, its = outs[schedule]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_batch_device(syn, err, conv, None, its)
            torch.cuda.synchronize()
            if i >= warmup:
                times[schedule].append(time.perf_counter() - t0)
    info = decs["layered"].info()
    print(f"{title}: batch {B}, max_iters {iters}; tier {info.kernel}, S {info.tile_syndromes}, K {info.layers}", flush=True)
    for schedule in ("flooding", "layered"):
        ts = np.array(times[schedule])
        _, conv, its = outs[schedule]
        mean_its = float(its.float().mean())
        print(f"  {schedule:8s} median {np.median(ts) * 1e3:9.3f} ms, spread {(ts.max() - ts.min()) * 1e3:8.3f} ms; mean iterations {mean_its:6.2f},"
              f" converged {float((conv != 0).float().mean()) * 100:6.2f} %; {np.median(ts) * 1e3 / max(mean_its, 1e-9):8.3f} ms per mean iteration",
              flush=True)
    both = (outs["flooding"][1] != 0) & (outs["layered"][1] != 0)
    if bool(both.any()):
        f_its, l_its = float(outs["flooding"][2][both].float().mean()), float(outs["layered"][2][both].float().mean())
        print(f"  on the {int(both.sum())} columns both converge on: mean iterations {f_its:.2f} -> {l_its:.2f};"
              f" layered / flooding time {np.median(times['layered']) / np.median(times['flooding']):.2f} x", flush=True)
    ok = True
    if n <= 2000:
        from layered_model import LayeredMinSumModel
        from minsum_model import MinSumModel

        sub = syn[:32].cpu().numpy()
        prior = decs["flooding"].channel_llr
        for schedule, model in (("flooding", MinSumModel(H, prior, iters)), ("layered", LayeredMinSumModel(H, prior, iters))):
            merr, mconv, mits, _ = model.decode(sub)
            err, conv, its = outs[schedule]
            ok = ok and (np.array_equal(err[:32].cpu().numpy(), merr) and np.array_equal(conv[:32].cpu().numpy(), mconv)
                         and np.array_equal(its[:32].cpu().numpy(), mits))
        print(f"  the first 32 columns of both decodes equal the models: {'yes' if ok else 'NO'}", flush=True)
    for dec in decs.values():
        dec.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_probe.txt"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=CASES, help="run this case here (what the probe starts once per case)")
    args = ap.parse_args()
    assert args.reps >= 1 and args.warmup >= 1
    if args.case:
        sys.exit(0 if run_case(args.case, args.warmup, args.reps) else 1)
    lines = [f"layered_probe: one box, a process per case, {args.reps} repetitions after {args.warmup} warm-up(s) per decoder, the schedules in turn;"
             " time = host clock around one device-entry call + device synchronise; spread = max - min"]
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
