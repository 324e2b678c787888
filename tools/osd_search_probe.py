#!/usr/bin/env python
"""The standard rule of the OSD step (osd_method=, ldpc_osd_set_search) next to what the library had before it: the
time of its kernel against the reference-rule device kernel, and the logical failure rate it buys.

  python tools/osd_search_probe.py --reference-lib PATH/libldpc_mi355x.so [--out profiles/osd_search_probe.txt]

Models, batch 65,536 each: BB-72 H_X with errors at 0.06 (one rate: prior weights are then a multiple of the count), and
the phenomenological BB-72 model of R = 6 rounds, data errors at 0.01 and measurement errors at 0.02 (216 detectors x
612 mechanisms, two rates).

Kernel time.  Inputs: the syndromes of Trials.sample / sample_rates (seed 1) and MinSumDecoder(30)'s hard decisions and
LLRs on them, the same in every case.  One ldpc_osd_postprocess_batch_device call between two events on the stream, one
untimed call first, median and spread (max - min) over `reps`; on the whole batch and on its unconverged columns alone
(the reference rule at order > 0 has no shortcut for a converged column, the standard rule has one at every order).
The reference-rule kernel is timed from --reference-lib, a build of the commit BEFORE the standard rule was added, bound
here by hand, so that the code it is compared with is not the code under test.

Logical failure rate.  run_trials, 65,536 trials of seed 1, block errors (the guess misses the syndrome or differs from
the error by a logical operator) of: min-sum(30); + reference-rule OSD-0; + standard OSD-0 (candidate 0 alone); + CS-10
with Hamming weights; + CS-10 with prior weights; relay at its defaults.

Every case runs in a process of its own (this script starts itself once per case, one at a time, and stops at the first
case that fails).  Measured, not tuned; no threshold."""
import argparse
import ctypes
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
MODELS = {"bb72": "BB-72 H_X, errors at 0.06", "phen6": "phenomenological BB-72, R = 6, p = 0.01, q = 0.02"}
RATE_CASES = {"minsum": "min-sum(30)", "ref0": "min-sum(30) + reference OSD-0", "std0": "min-sum(30) + standard OSD-0",
              "cs10h": "min-sum(30) + CS-10, Hamming weights", "cs10p": "min-sum(30) + CS-10, prior weights", "relay": "relay (defaults)"}
TIME_CASES = {"ref": "reference rule (build before this change)", "exh": "standard rule, exhaustive", "cs": "standard rule, combination sweep"}


def model_of(key):
    """-> (H csc, logicals, rates [n])"""
    HX, HZ = ldpc.codes.bivariate_bicycle_72_12_6()
    Lz = ldpc.codes.css_logicals(HX, HZ)[1]
    if key == "bb72":
        return sp.csc_matrix(np.asarray(sp.csc_matrix(HX).todense(), dtype=np.uint8)), Lz, np.full(72, 0.06)
    dem = ldpc.phenomenological(HX, Lz, 6, 0.01, 0.02)
    return sp.csc_matrix(dem.H), dem.L, np.asarray(dem.rates, dtype=np.float64)


def rate_case(key, case):
    import torch

    H, L, rates = model_of(key)
    if case == "relay":
        dec = ldpc.RelayMinSumDecoder(H, channel_probs=rates)
    else:
        dec = ms = ldpc.MinSumDecoder(H, channel_probs=rates, max_iters=30)
        kw = {"ref0": dict(osd_order=0), "std0": dict(osd_order=0, osd_method="exhaustive"),
              "cs10h": dict(osd_order=10, osd_method="combination_sweep"),
              "cs10p": dict(osd_order=10, osd_method="combination_sweep", osd_weights="priors")}.get(case)
        if kw is not None:
            dec = ldpc.BeliefPropagationOSDDecoder(H, bp_decoder=ms, osd="device", **kw)
    t0 = time.perf_counter()
    r = ldpc.run_trials(dec, BATCH, per=rates, batch=BATCH, seed=1, logicals=L)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(dict(block_errors=r.block_errors, syndrome_mismatches=r.syndrome_mismatches,
                                      not_converged=r.not_converged, trials=r.trials, wall_s=time.perf_counter() - t0,
                                      device=torch.cuda.get_device_name(0))), flush=True)


def _bind_reference(path):
    """The five ldpc_osd_* entries of the build before this change, by hand (it lacks the symbols the package binds)."""
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L = ctypes.CDLL(path)
    for name, args in (("ldpc_osd_create", [i64, i64, i64, vp, vp, i64, ctypes.POINTER(vp)]), ("ldpc_osd_destroy", [vp]),
                       ("ldpc_osd_device_prepare", [vp, i32, i32]), ("ldpc_osd_device_kernel", [vp]),
                       ("ldpc_osd_postprocess_batch_device", [vp, i64, vp, vp, vp, vp, vp])):
        getattr(L, name).restype, getattr(L, name).argtypes = i32, args
    assert not hasattr(L, "ldpc_osd_set_search"), "--reference-lib must be a build from before the standard rule"
    return L


def time_case(key, order, case, reps, reference_lib):
    import torch

    H, L, rates = model_of(key)
    s, n = H.shape
    tr = ldpc.Trials(H, L)
    tr.set_rates(rates)
    _, syn = tr.sample_rates(BATCH, seed=1)
    ms = ldpc.MinSumDecoder(H, channel_probs=rates, max_iters=30)
    err = torch.empty((BATCH, n), dtype=torch.uint8, device=syn.device)
    conv = torch.empty(BATCH, dtype=torch.uint8, device=syn.device)
    llr = torch.empty((BATCH, n), dtype=torch.float64, device=syn.device)
    ms.decode_batch_device(syn, err, conv, llr, None)
    idx = torch.nonzero(conv == 0, as_tuple=False).flatten()
    sets = {"whole batch": (syn, err, llr), "unconverged columns": (syn[idx].contiguous(), err[idx].contiguous(), llr[idx].contiguous())}
    if case == "ref":
        R = _bind_reference(reference_lib)
        M = sp.csc_matrix(H)
        M.sort_indices()
        colptr, rowval = M.indptr.astype(np.int64), M.indices.astype(np.int64)
        h = ctypes.c_void_p()
        assert R.ldpc_osd_create(s, n, rowval.size, colptr.ctypes.data, rowval.ctypes.data, order, ctypes.byref(h)) == 0
        assert R.ldpc_osd_device_prepare(h, 0, 0) == 0
        tier = R.ldpc_osd_device_kernel(h)

        def call(a, b, c, out):
            assert R.ldpc_osd_postprocess_batch_device(h, a.shape[0], a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream) == 0
    else:
        post = ldpc.OSDPostProcessor(H, order, method="exhaustive" if case == "exh" else "combination_sweep")
        tier = post.prepare_device(0)

        def call(a, b, c, out):
            post.postprocess_device(a, b, c, out=out)
    res = dict(tier=int(tier), unconverged=int(idx.numel()), device=torch.cuda.get_device_name(0))
    for name, (a, b, c) in sets.items():
        out = torch.empty_like(b)
        call(a, b, c, out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(a, b, c, out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[name] = (float(np.median(ts)), float(max(ts) - min(ts)))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osd_search_probe.txt"))
    ap.add_argument("--reference-lib", help="libldpc_mi355x.so built from the commit before the standard rule")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds a case may take")
    ap.add_argument("--case", nargs="+", help="run one case in this process (internal)")
    args = ap.parse_args()
    if args.case:
        if args.case[0] == "rate":
            return rate_case(args.case[1], args.case[2])
        return time_case(args.case[1], int(args.case[2]), args.case[3], args.reps, args.reference_lib)
    assert args.reference_lib and os.path.exists(args.reference_lib), "--reference-lib: a build of the parent commit is needed"
    lines = []

    def say(x=""):
        print(x, flush=True)
        lines.append(x)

    def run(case):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--reference-lib", args.reference_lib,
                            "--case"] + [str(c) for c in case], capture_output=True, text=True, timeout=args.limit)
        got = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not got:   # nothing more runs on a device that has just failed a case
            say(f"{case}: FAILED (exit {p.returncode})\n{p.stderr[-2000:]}")
            raise SystemExit(1)
        return json.loads(got[-1][7:])

    try:
        first = True
        for key, title in MODELS.items():
            for order in (0, 10):
                for case, name in TIME_CASES.items():
                    if order == 0 and case == "cs":
                        continue   # (the sweep at order 0 still has its K single flips: not the work of OSD-0)
                    r = run(("time", key, order, case))
                    if first:
                        say(f"osd_search_probe: {r['device']}, batch {BATCH}, {args.reps} repetitions after 1 warm-up, every case in a process"
                            " of its own; kernel time = two events around one device-entry call; spread = max - min")
                        first = False
                    if case == "ref":
                        say(f"{title}: OSD kernel alone, order {order}, {r['unconverged']} of {BATCH} columns unconverged after min-sum(30)")
                    w, u = r["whole batch"], r["unconverged columns"]
                    say(f"  {name:42s} tier {r['tier']}  whole batch {w[0]:9.3f} ms (spread {w[1]:7.3f});"
                        f" unconverged columns {u[0]:9.3f} ms (spread {u[1]:7.3f})")
            say(f"{title}: logical failure rate, {BATCH} trials")
            for case, name in RATE_CASES.items():
                r = run(("rate", key, case))
                say(f"  {name:38s} {r['block_errors'] / r['trials']:.4f} ({r['block_errors']} of {r['trials']}; {r['syndrome_mismatches']} miss the"
                    f" syndrome; {r['not_converged']} unconverged; run {r['wall_s']:.2f} s)")
    finally:   # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
