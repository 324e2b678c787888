#!/usr/bin/env python
"""Times one joint X/Z decode (ldpcdecoders.jl_amd/pauli.py: PauliMinSumDecoder.decode_batch_device) against the two
MinSumDecoder decodes it replaces, on the same sampled trials, and scores both.

  python tools/pauli_probe.py [--out profiles/pauli_probe.txt] [--warmup 2] [--reps 7]

Cases (every one in a process of its own, started from here), 65,536 trials as one batch, 30 iterations, alpha 0.75,
flooding schedule on both sides of the comparison:
  bb72  BB-72 under depolarizing noise 0.06: the joint decoder on chip (S = 32)
  hgp   the hypergraph product of the (84, 6, 3) Gallager matrix (n = 8820, 3528 + 3528 checks) under depolarizing noise
        0.02: 190,512 B a syndrome, so the joint decoder takes the unlimited tier; each min-sum side is on chip (S = 1)
The joint decoder is built from p (priors log(P(I) / P(W))), each min-sum at the marginal rate 2 p / 3.  Every time is a
pair of device events around the decode (for the independent pair: around both calls), after `warmup` untimed rounds;
the two are timed in turn, repetition by repetition, so that both see the same machine; median and spread (max - min)
over `reps`.  The counts are those of ldpc_css_trials_score_device on the outputs of the last repetition.  Nothing is
tuned here and no ratio is asserted."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("bb72", "hgp")
BATCH, ITERS = 1 << 16, 30


def code_of(ldpc, name):
    import scipy.sparse as sp

    if name == "bb72":
        Hx, Hz = (sp.csc_matrix(np.asarray(M, dtype=np.uint8)) for M in ldpc.codes.bivariate_bicycle_72_12_6())
        return "BB-72", Hx, Hz, 0.06
    Hx, Hz = ldpc.codes.hypergraph_product(ldpc.parity_check_matrix(84, 6, 3))
    return "HGP(84,6,3) n=8820", Hx, Hz, 0.02


def run_case(name, warmup, reps):
    import torch

    import ldpcdecoders_jl_amd as ldpc

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    title, Hx, Hz, p = code_of(ldpc, name)
    n, B = Hx.shape[1], BATCH
    tr = ldpc.CSSTrials(Hx, Hz, logicals=ldpc.codes.css_logicals(Hx, Hz))
    ex, ez, sx, sz = tr.sample(B, p, seed=1)
    joint = ldpc.PauliMinSumDecoder(Hx, Hz, p, ITERS)
    side_x, side_z = ldpc.MinSumDecoder(Hz, 2 * p / 3, ITERS), ldpc.MinSumDecoder(Hx, 2 * p / 3, ITERS)   # Hz sees the X parts
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")   # noqa: E731
    out = {k: (u8(B, n), u8(B, n), u8(B), u8(B), torch.empty(B, dtype=torch.int32, device="cuda"),
               torch.empty(B, dtype=torch.int32, device="cuda")) for k in ("joint", "independent")}

    def run_joint(o):
        joint.decode_batch_device(sx, sz, o[0], o[1], o[2], None, o[4])

    def run_independent(o):
        side_x.decode_batch_device(sz, o[0], o[2], None, o[4])
        side_z.decode_batch_device(sx, o[1], o[3], None, o[5])

    calls = {"joint": run_joint, "independent": run_independent}
    times = {k: [] for k in calls}
    for i in range(warmup + reps):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(out[k])
            b.record()
            b.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    print(f"{title}, depolarizing {p}: batch {B}, max_iters {ITERS}; joint tier {joint.kernel}, S {joint.tile_syndromes}, grid {joint.last_grid};"
          f" min-sum sides tier {side_x.kernel} / {side_z.kernel}, S {side_x.info().tile_syndromes} / {side_z.info().tile_syndromes}", flush=True)
    base = float(np.median(times["independent"]))
    for k in calls:
        o = out[k]
        _, counts = tr.score(o[0], o[1], ex, ez, want_flags=False)
        c = counts.cpu().tolist()
        conv = (o[2] != 0) if k == "joint" else ((o[2] != 0) & (o[3] != 0))
        its = o[4].float().mean() if k == "joint" else (o[4].float().mean() + o[5].float().mean()) / 2
        ts = np.array(times[k])
        print(f"  {k:11s}: median {np.median(ts):9.3f} ms, spread {ts.max() - ts.min():7.3f} ms; {np.median(ts) / base:5.2f} x independent;"
              f" logical failure rate {c[3] / c[0]:.5f} (X {c[4] / c[0]:.5f}, Z {c[5] / c[0]:.5f}), block {c[1] / c[0]:.5f},"
              f" converged {float(conv.float().mean()) * 100:.2f} %, mean iterations {float(its):.2f}", flush=True)
    for d in (joint, side_x, side_z, tr):
        d.close()
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--case", choices=CASES, help="run this case here (what the probe starts once per case)")
    args = ap.parse_args()
    assert args.reps >= 1 and args.warmup >= 1
    if args.case:
        sys.exit(0 if run_case(args.case, args.warmup, args.reps) else 1)
    lines = [f"pauli_probe: one box, a process per case, {args.reps} repetitions after {args.warmup} warm-up(s), joint and independent in turn;"
             " time = device events around one joint decode / around the two min-sum decodes it replaces, on the same sampled trials;"
             " spread = max - min; rates = counts of the trial score over the batch"]
    print(lines[0], flush=True)
    all_ok = True
    for name in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--warmup", str(args.warmup), "--reps", str(args.reps)],
                             capture_output=True, text=True, timeout=420)
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
