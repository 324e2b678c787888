#!/usr/bin/env python
"""Times the per-bit sample step and detector-error-model runs (ldpcdecoders.jl_amd/trials.py, dem.py) and checks what
it timed.

  python tools/dem_trials_probe.py [--out profiles/dem_trials_probe.txt] [--warmup 2] [--reps 5] [--trials 262144]

1. Trials.sample_rates against Trials.sample of the same build, on the same handle, with every rate equal to the `per`
   of the uniform call (so both do the same work and must write the same bytes): (16384, 8, 4) batch 65,536;
   parity_check_matrix(1000, 10, 9) batch 2^18; the phenomenological model of BB-72 H_X at R = 6 (n = 612, s = 216)
   batch 2^20, there also at the model's own rates.  The two are timed in turn, repetition by repetition.  The ratio of
   the medians is the price of the table; no bound is set on it here.
2. run_dem_trials of RelayMinSumDecoder and of MinSumDecoder (channel_probs = the model's rates) on that model: time,
   the share of converged columns and the logical failure rate.
One process per case (this one starts them and never touches the GPU itself).  Every time is a host clock around one
call that ends in a device synchronise, after `warmup` untimed calls; median and spread (max - min) over `reps`.  A column
sample of every timed per-bit output is compared with the CPU model (tests/dem_model.py).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("sample:big", "sample:1000", "sample:dem", "run:relay", "run:minsum")
P_DATA, Q_MEAS, ROUNDS = 0.01, 0.02, 6


def median_spread(ts):
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.max() - ts.min())


def bb72_dem(ldpc):
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    _, Lz = ldpc.codes.css_logicals(Hx, Hz)
    return ldpc.phenomenological(Hx, Lz, ROUNDS, P_DATA, Q_MEAS)


def sample_case(case, args, say):
    import torch

    import dem_model as dm
    import ldpcdecoders_jl_amd as ldpc
    import trials_model as tm

    dev = torch.device("cuda", 0)
    own = None
    if case == "sample:big":
        name, H, per, B = "(16384,8,4)", ldpc.codes.parity_check_csc(16384, 8, 4), 0.02, 1 << 16
    elif case == "sample:1000":
        name, H, per, B = "(1000,10,9)", ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 1 << 18
    else:
        dem = bb72_dem(ldpc)
        name, H, per, B, own = f"phenomenological BB-72 H_X, R = {ROUNDS}", dem.H, P_DATA, 1 << 20, dem.rates
    s, n = H.shape
    t = ldpc.Trials(H)
    err = torch.empty((B, n), dtype=torch.uint8, device=dev)
    syn = torch.empty((B, s), dtype=torch.uint8, device=dev)
    err2, syn2 = torch.empty_like(err), torch.empty_like(syn)
    t.set_rates(np.full(n, per))
    uniform = lambda: t.sample(B, per, seed=1, out=(err, syn))            # noqa: E731
    per_bit = lambda: t.sample_rates(B, seed=1, out=(err2, syn2))         # noqa: E731
    for _ in range(args.warmup):
        uniform()
        per_bit()
    torch.cuda.synchronize()
    tu, tp = [], []
    for _ in range(args.reps):                                            # in turn, so that both see the same machine
        for fn, ts in ((uniform, tu), (per_bit, tp)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    (u_med, u_spread), (p_med, p_spread) = median_spread(tu), median_spread(tp)
    same = torch.equal(err, err2) and torch.equal(syn, syn2)
    idx = np.unique(np.linspace(0, B - 1, 48).astype(np.int64))
    want = np.concatenate([dm.sample(np.full(n, per), 1, 1, int(i)) for i in idx])
    ok = same and np.array_equal(err2[idx].cpu().numpy(), want) and np.array_equal(syn2[idx].cpu().numpy(), tm.syndromes(H, want))
    say(f"{name}: n {n}, s {s}, batch {B}, every rate {per}, tier {t.kernel}")
    say(f"  sample        (errors + syndromes): median {u_med * 1e3:.3f} ms, spread {u_spread * 1e3:.3f} ms")
    say(f"  sample_rates  (errors + syndromes): median {p_med * 1e3:.3f} ms, spread {p_spread * 1e3:.3f} ms"
        f"  -> {p_med / u_med:.3f} x the uniform sample, {B * (n + s) / p_med / 1e12:.3f} TB/s written;"
        f" equal to the uniform sample in every byte and to the model in {len(idx)} columns: {'yes' if ok else 'NO'}")
    if own is not None:
        t.set_rates(own)
        for _ in range(args.warmup):
            per_bit()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            per_bit()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        o_med, o_spread = median_spread(ts)
        want = np.concatenate([dm.sample(own, 1, 1, int(i)) for i in idx])
        ok2 = np.array_equal(err2[idx].cpu().numpy(), want) and np.array_equal(syn2[idx].cpu().numpy(), tm.syndromes(H, want))
        ok = ok and ok2
        say(f"  sample_rates at the model's rates ({P_DATA} data, {Q_MEAS} measurement): median {o_med * 1e3:.3f} ms,"
            f" spread {o_spread * 1e3:.3f} ms; equal to the model in {len(idx)} columns: {'yes' if ok2 else 'NO'}")
    t.close()
    return ok


def run_case(case, args, say):
    import torch

    import ldpcdecoders_jl_amd as ldpc

    dem = bb72_dem(ldpc)
    if case == "run:relay":
        name, dec = "RelayMinSumDecoder (30 + 8 x 20 iterations)", ldpc.RelayMinSumDecoder(dem.H, None, 30, channel_probs=dem.rates, legs=9, leg_iters=20)
    else:
        name, dec = "MinSumDecoder (50 iterations)", ldpc.MinSumDecoder(dem.H, None, 50, channel_probs=dem.rates)
    B = 1 << 16
    res = [None]

    def loop():
        res[0] = ldpc.run_dem_trials(dem, dec, args.trials, batch=B, seed=1)

    for _ in range(args.warmup):
        loop()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        loop()                                                            # (ends in the read-back of the counts)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med, spread = median_spread(ts)
    r = res[0]
    say(f"run_dem_trials, phenomenological BB-72 H_X, R = {ROUNDS} (n {dem.num_mechanisms}, s {dem.num_detectors}, {dem.num_observables}"
        f" observables), {name}, {args.trials} trials in batches of {B}:")
    say(f"  median {med * 1e3:.1f} ms, spread {spread * 1e3:.1f} ms -> {args.trials / med / 1e6:.2f} M trials/s; converged"
        f" {1.0 - r.not_converged_rate:.5f}, syndrome reproduced {1.0 - r.syndrome_mismatch_rate:.5f},"
        f" logical failure rate {r.logical_error_rate:.3e} ({r.logical_errors} of {r.trials})")
    dec.close()
    return r.trials == args.trials


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dem_trials_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=1 << 18)
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, help="run this case alone, in this process (what the probe starts per case)")
    args = ap.parse_args()
    if args.case:
        import torch

        import ldpcdecoders_jl_amd as ldpc

        assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
        say = lambda x="": print(x, flush=True)                           # noqa: E731
        ok = (sample_case if args.case.startswith("sample") else run_case)(args.case, args, say)
        say(f"case {args.case} on {torch.cuda.get_device_name(0)}: {'ok' if ok else 'FAILED'}")
        sys.exit(0 if ok else 1)
    lines = [f"dem_trials_probe: one box, one process per case, {args.reps} repetitions after {args.warmup} warm-ups; "
             "time = host clock around one call + device synchronise; spread = max - min"]
    print(lines[0], flush=True)
    all_ok = True
    for case in CASES:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--warmup", str(args.warmup),
                                  "--reps", str(args.reps), "--trials", str(args.trials)], stdout=subprocess.PIPE, text=True,
                                 timeout=args.case_timeout)
            status, text = out.returncode, out.stdout
        except subprocess.TimeoutExpired as e:
            status, text = "time limit", (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(text, end="", flush=True)
        lines += text.splitlines()
        if status != 0:
            all_ok = False
            lines.append(f"case {case}: exit status {status}")
            print(lines[-1], flush=True)
            break                                                         # nothing more is started on a GPU after a failure
    lines.append(f"all cases: {'ok' if all_ok else 'FAILED'}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all_ok, "a case failed (see above)"


if __name__ == "__main__":
    main()
