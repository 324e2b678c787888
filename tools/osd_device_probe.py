#!/usr/bin/env python3
"""BP+OSD with the ordered-statistics step on the host (default) and on the device (osd="device"): time of one
BeliefPropagationOSDDecoder.batchdecode_device call, host clock around the call + device synchronise, one warm-up and
REPS repetitions each, median and spread ((max - min) / median), both forms in the same run.

    python tools/osd_device_probe.py              # the five cases -> stdout (committed as profiles/osd_device_probe.txt)
    python tools/osd_device_probe.py --kernel c   # only the device form of one case, a few calls: the run to put under
                                                  # `rocprofv3 --kernel-trace --stats` for the OSD kernel's own time
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ldpcdecoders_jl_amd as ldpc  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))


def bb72():
    return ldpc.codes.bivariate_bicycle_72_12_6()[0]


# name, H, decoder per, error rate, iterations, batch, osd_order
CASES = {
    "a": ("(a) BB-72 config 5 as worded: errors at 0.005, order 0", bb72, 0.005, 0.005, 50, 1 << 20, 0),
    "b": ("(b) BB-72, errors at 0.04, order 0", bb72, 0.005, 0.04, 50, 1 << 20, 0),
    "c": ("(c) BB-72, errors at 0.005, order 3", bb72, 0.005, 0.005, 50, 1 << 20, 3),
    "d": ("(d) BB-72, errors at 0.005, order 10", bb72, 0.005, 0.005, 50, 1 << 16, 10),
    "e": ("(e) parity_check_csc(1000,10,9), per 0.05, order 0", lambda: ldpc.codes.parity_check_csc(1000, 10, 9), 0.05, 0.05, 50, 4096, 0),
}


def timed(dec, syn, reps):
    dec.batchdecode_device(syn)   # warm-up (allocations, the two-pass / one-pass choice of order 0)
    torch.cuda.synchronize()
    ts, sent = [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        err, conv, sent = dec.batchdecode_device(syn)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max()), sent, err


def main():
    only_kernel = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--kernel" else None
    print(f"osd_device_probe: {torch.cuda.get_device_name(0)}, reps {REPS} (+1 warm-up), host threads {os.cpu_count()}"
          f" (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')})")
    for key, (name, mk, per, rate, iters, B, order) in CASES.items():
        if only_kernel and key != only_kernel:
            continue
        H = mk()
        n = H.shape[1]
        syn = torch.from_numpy(ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, B, rate, seed=9))).to("cuda:0")
        dev = ldpc.BeliefPropagationOSDDecoder(H, per, iters, osd_order=order, osd="device")
        if only_kernel:
            for _ in range(3):
                dev.batchdecode_device(syn)
            torch.cuda.synchronize()
            print(f"{name}: 3 device-form calls, tier {dev._osd.kernel}")
            continue
        host = ldpc.BeliefPropagationOSDDecoder(H, per, iters, osd_order=order)
        hm, hlo, hhi, hsent, herr = timed(host, syn, REPS)
        dm, dlo, dhi, dsent, derr = timed(dev, syn, REPS)
        differ = int((herr != derr).any(dim=1).sum())
        print(f"{name}: batch {B}, sent to OSD {dsent} (host form {hsent}), device tier {dev._osd.kernel}")
        print(f"    osd=\"host\"   median {hm:9.3f} ms  min {hlo:9.3f}  max {hhi:9.3f}  spread {100 * (hhi - hlo) / hm:5.1f} %")
        print(f"    osd=\"device\" median {dm:9.3f} ms  min {dlo:9.3f}  max {dhi:9.3f}  spread {100 * (dhi - dlo) / dm:5.1f} %")
        print(f"    host / device = {hm / dm:.2f}; estimates differ on {differ} of {B} syndromes")
        del host, dev, herr, derr


if __name__ == "__main__":
    main()
