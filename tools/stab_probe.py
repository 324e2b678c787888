#!/usr/bin/env python
"""Times one stabilizer min-sum decode (ldpcdecoders.jl_amd/stabilizer.py: StabilizerMinSumDecoder.decode_batch_device)
against what a user had before it, on the same sampled trials, and scores both.

  python tools/stab_probe.py [--out profiles/stab_probe.txt] [--warmup 2] [--reps 7]

Cases (every one in a process of its own, started from here), 65,536 trials as one batch, 30 iterations, alpha 0.75:
  css       BB-72 as a CSS input ([Hx; 0], [0; Hz]) under depolarizing noise 0.06, against PauliMinSumDecoder on (Hx, Hz):
            the outputs are equal (asserted); the state of a syndrome is 3 n against 2 n words of totals
  deformed  BB-72 under the single-qubit Cliffords of default_rng(7) (all three edge types), depolarizing 0.06, against
            MinSumDecoder on the binary symplectic matrix [Sz | Sx] with the marginal priors (px + py, py + pz)
  biased    the same code under (px, py, pz) = (0.005, 0.005, 0.08), the same comparison
  xzzx      xzzx_surface_code(5) under (0.004, 0.004, 0.10), the same comparison
Every time is a pair of device events around the decode, after `warmup` untimed rounds; the two decoders are timed in
turn, repetition by repetition, so that both see the same machine; median and spread (max - min) over `reps`.  The counts
are those of the binary trial score over [Sz | Sx] with the logical rows [LSz | LSx] on the outputs of the last
repetition.  Measured, not tuned: no ratio is asserted."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("css", "deformed", "biased", "xzzx")
BATCH, ITERS = 1 << 16, 30


def code_of(ldpc, name):
    import scipy.sparse as sp

    codes = ldpc.codes
    if name == "xzzx":
        Sx, Sz = codes.xzzx_surface_code(5)
        return "XZZX surface code d=5", None, Sx, Sz, (0.004, 0.004, 0.10)
    Hx, Hz = (sp.csc_matrix(np.asarray(M, dtype=np.uint8)) for M in codes.bivariate_bicycle_72_12_6())
    if name == "css":
        Sx, Sz = codes.clifford_deform(Hx, Hz, np.zeros(72, dtype=np.int64))
        return "BB-72 as a CSS input", (Hx, Hz), Sx, Sz, 0.06
    Sx, Sz = codes.clifford_deform(Hx, Hz, np.random.default_rng(7).integers(0, 6, 72))
    return "BB-72 deformed (rng 7)", None, Sx, Sz, (0.06 if name == "deformed" else (0.005, 0.005, 0.08))


def run_case(name, warmup, reps):
    import scipy.sparse as sp
    import torch

    import ldpcdecoders_jl_amd as ldpc
    from ldpcdecoders_jl_amd.css_trials import pauli_rates

    assert ldpc._capi.lib().ldpc_device_count() > 0, "no gfx950 device: nothing to measure"
    title, css, Sx, Sz, p = code_of(ldpc, name)
    r, n = Sx.shape
    B = BATCH
    LSx, LSz = ldpc.codes.stabilizer_logicals(Sx, Sz)
    sampler = ldpc.CSSTrials(Sx, Sz, logicals=False, check=False)
    scorer = ldpc.Trials(sp.hstack([Sz, Sx]), sp.hstack([sp.csc_matrix(LSz), sp.csc_matrix(LSx)]))
    ex, ez, sx, sz = sampler.sample(B, p, seed=1)
    syn = sx ^ sz
    err = torch.cat((ex, ez), dim=1)
    stab = ldpc.StabilizerMinSumDecoder(Sx, Sz, p, ITERS)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")   # noqa: E731
    i32 = lambda: torch.empty(B, dtype=torch.int32, device="cuda")             # noqa: E731
    out = {"stabilizer": (u8(B, n), u8(B, n), u8(B), i32())}
    calls = {"stabilizer": lambda o: stab.decode_batch_device(syn, o[0], o[1], o[2], None, o[3])}
    if css is not None:
        other_name = "pauli"
        other = ldpc.PauliMinSumDecoder(css[0], css[1], p, ITERS)
        rx = css[0].shape[0]
        hx_syn, hz_syn = syn[:, :rx].contiguous(), syn[:, rx:].contiguous()
        out[other_name] = (u8(B, n), u8(B, n), u8(B), i32())
        calls[other_name] = lambda o: other.decode_batch_device(hx_syn, hz_syn, o[0], o[1], o[2], None, o[3])
        other_what = f"Pauli tier {other.kernel}, S {other.tile_syndromes}, {4 * (2 * n) } B of totals a syndrome"
    else:
        other_name = "binary"
        px, py, pz = pauli_rates(p)
        probs = np.concatenate([np.full(n, px + py), np.full(n, py + pz)])
        other = ldpc.MinSumDecoder(sp.csc_matrix(sp.hstack([Sz, Sx])), None, ITERS, channel_probs=probs)
        out[other_name] = (u8(B, 2 * n), None, u8(B), i32())
        calls[other_name] = lambda o: other.decode_batch_device(syn, o[0], o[2], None, o[3])
        other_what = f"binary min-sum on [Sz | Sx] tier {other.kernel}, S {other.info().tile_syndromes}"
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
    print(f"{title}, noise {p}: batch {B}, max_iters {ITERS}, r {r}, n {n}; stabilizer tier {stab.kernel}, S {stab.tile_syndromes}, grid {stab.last_grid},"
          f" {4 * 3 * n} B of totals a syndrome; {other_what}", flush=True)
    base = float(np.median(times[other_name]))
    for k in calls:
        o = out[k]
        guess = o[0] if o[1] is None else torch.cat((o[0], o[1]), dim=1)
        _, counts = scorer.score(guess, err, want_flags=False)
        c = counts.cpu().tolist()
        ts = np.array(times[k])
        print(f"  {k:10s}: median {np.median(ts):9.3f} ms, spread {ts.max() - ts.min():7.3f} ms; {np.median(ts) / base:5.2f} x {other_name};"
              f" logical failure rate {c[3] / c[0]:.5f}, block {c[1] / c[0]:.5f}, syndrome mismatch {c[2] / c[0]:.5f},"
              f" converged {float((o[2] != 0).float().mean()) * 100:.2f} %, mean iterations {float(o[3].float().mean()):.2f}", flush=True)
    if css is not None:
        a, b = out["stabilizer"], out["pauli"]
        equal = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        print(f"  outputs equal (gx, gz, converged, iters): {equal}", flush=True)
        if not equal:
            return False
    for d in (stab, other, sampler, scorer):
        d.close()
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stab_probe.txt"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--case", choices=CASES, help="run this case here (what the probe starts once per case)")
    args = ap.parse_args()
    assert args.reps >= 1 and args.warmup >= 1
    if args.case:
        sys.exit(0 if run_case(args.case, args.warmup, args.reps) else 1)
    lines = [f"stab_probe: one box, a process per case, {args.reps} repetitions after {args.warmup} warm-up(s), the two decoders in turn;"
             " time = device events around one decode of the batch, on the same sampled trials; spread = max - min;"
             " rates = counts of the binary trial score over [Sz | Sx] with the logical rows [LSz | LSx]; measured, not tuned"]
    print(lines[0], flush=True)
    all_ok = True
    for name in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--warmup", str(args.warmup), "--reps", str(args.reps)],
                             capture_output=True, text=True, timeout=240)
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
