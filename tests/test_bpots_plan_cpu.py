"""The kernel, tile width, LDS budget and register buckets of the BP-OTS decoder without a GPU: ldpc_debug_bpots_plan
(csrc/bpots_plan.hpp ots_plan(), the function ldpc_bpots_create calls) against the byte formulas restated here from the
header comment of include/ldpc_mi355x_debug.h, over a grid of sizes around every threshold; the (3,6)-regular sizes at
which tests/test_gpu_bpots_paths.py runs every tile width, as literal rows; the refusals; wide graphs and force_node.

One thing this pins on purpose: the 156 KiB budget is only ever taken with S = 1 -- at n = 612, S = 2 would
fit 156 KiB as well, and the plan answers S = 1.  Whether that is the best choice is a question for a measured change."""
import ctypes
import os
import shutil
import subprocess

import pytest

import ldpcdecoders_jl_amd as ldpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 5
KIB76, KIB156 = 76 * 1024, 156 * 1024


def lds_bytes(s, n, nnz, S):
    """Dynamic LDS of the LDS-resident kernel for S syndromes per workgroup (the debug header's formula)."""
    return 8 * S * nnz + 12 * S * n + 24 * n + 32 * s + 2112 + 24 * 512 + 2 * (s + n + 2 + 2 * nnz) + 32


def node_lds_bytes(s, n):
    return ((s + 3 * n + 15) // 16) * 16 + 4 * s + 28 * 1024 + 64


def model_plan(s, n, nnz, cdeg, bdeg, force_node=0):
    """(kernel, S, lds bytes, budget KiB, DC, DV) by the rule in words: the largest S <= 64 that fits 76 KiB, else S = 1 in
    156 KiB, else the node kernel, else the unlimited one."""
    wide = cdeg > 32 or bdeg > 16
    buckets = (8 if cdeg <= 8 else 32, 4 if bdeg <= 4 else 16)
    if not force_node and not wide and max(s, n, nnz) < 65535:
        for S in (64, 32, 16, 8, 4, 2, 1):
            if lds_bytes(s, n, nnz, S) + 8192 <= KIB76:
                return (2, S, lds_bytes(s, n, nnz, S), 76) + buckets
        if lds_bytes(s, n, nnz, 1) + 8192 <= KIB156:
            return (2, 1, lds_bytes(s, n, nnz, 1), 156) + buckets
    if wide or force_node >= 2 or node_lds_bytes(s, n) + 1024 > KIB156:
        return (5, 0, 0, 0, 0, 0)
    return (3, 0, node_lds_bytes(s, n), 0) + buckets


def lib_plan(s, n, nnz, cdeg, bdeg, force_node=0, experiments=False):
    """(status, kernel, S, lds bytes, budget KiB, DC, DV) of ldpc_debug_bpots_plan."""
    L = ldpc._capi.lib(experiments)
    k, logS, b, dc, dv = (ctypes.c_int32(-7) for _ in range(5))
    nbytes = ctypes.c_int64(-7)
    st = L.ldpc_debug_bpots_plan(s, n, nnz, cdeg, bdeg, force_node, ctypes.byref(k), ctypes.byref(logS), ctypes.byref(nbytes),
                                 ctypes.byref(b), ctypes.byref(dc), ctypes.byref(dv))
    if st != OK:
        assert (k.value, logS.value, nbytes.value, b.value, dc.value, dv.value) == (-7,) * 6   # nothing written on a refusal
        return (st,)
    assert (logS.value >= 0) == (k.value == 2)
    return (st, k.value, 1 << logS.value if logS.value >= 0 else 0, nbytes.value, b.value, dc.value, dv.value)


def regular(n):
    """Sizes of parity_check_csc(n, 6, 3)."""
    return n // 2, n, 3 * n, 6, 3


# n -> (S, budget KiB) for the (3,6)-regular code of n bits; S = 0: the node kernel
TABLE = {18: (64, 76), 36: (32, 76), 60: (16, 76), 120: (8, 76), 240: (4, 76), 360: (2, 76), 504: (1, 76), 606: (1, 76),
         612: (1, 156), 1200: (1, 156), 1500: (1, 156), 1512: (0, 0)}


@pytest.mark.parametrize("experiments", [False, True])
def test_the_table_of_tile_widths(experiments):
    for n, (S, budget) in TABLE.items():
        got = lib_plan(*regular(n), experiments=experiments)
        assert got[0] == OK and got[1] == (2 if S else 3) and got[2] == S and got[4] == budget and got[5:] == (8, 4), (n, got)
        assert got[1:] == model_plan(*regular(n)), n
    # the codes the table is about are what parity_check_csc builds
    for n in (18, 606, 1512):
        H = ldpc.codes.parity_check_csc(n, 6, 3)
        assert (H.shape[0], H.shape[1], H.nnz) == regular(n)[:3]
        assert ldpc.bpots.bpots_plan_of(H, experiments=experiments) == ldpc.bpots.bpots_plan(*regular(n), experiments=experiments)
    # the two edges, in bytes: what the budget test counts is the dynamic LDS plus 8192
    assert lib_plan(*regular(606))[3] + 8192 == 77774 <= KIB76 < lds_bytes(304, 608, 1824, 1) + 8192
    assert lib_plan(*regular(1500))[3] + 8192 == 159128 <= KIB156 < lds_bytes(756, 1512, 4536, 1) + 8192
    # the 156 KiB budget is only ever taken with S = 1, though S = 2 would fit it at n = 612 (see the module docstring)
    assert lds_bytes(306, 612, 1836, 2) + 8192 <= KIB156 and lib_plan(*regular(612))[2] == 1


def test_plan_equals_the_formula_around_every_threshold():
    seen = set()
    for wr, wc in ((6, 3), (8, 4), (4, 2), (32, 16), (9, 5), (12, 3), (6, 6)):
        sizes = set()
        for n in range(2 * wr, 2400, 2 * wr):
            s, nnz = n * wc // wr, n * wc
            # every n at which some width stops fitting, and its neighbours
            for S in (64, 32, 16, 8, 4, 2, 1):
                for budget in (KIB76, KIB156):
                    if lds_bytes(s, n, nnz, S) + 8192 <= budget < lds_bytes(s + wc * 2, n + 2 * wr, nnz + 2 * wr * wc, S) + 8192:
                        sizes.update((n - 2 * wr, n, n + 2 * wr, n + 4 * wr))
        assert len(sizes) >= 8, (wr, wc)
        for n in sorted(sizes | {2 * wr, 2400 // (2 * wr) * 2 * wr}):
            s, nnz = n * wc // wr, n * wc
            got = lib_plan(s, n, nnz, wr, wc)
            assert got == (OK,) + model_plan(s, n, nnz, wr, wc), (wr, wc, n, got)
            seen.add(got[1:3] + got[4:])
    # irregular sizes: nnz, s and n varied on their own, byte by byte across the 76 KiB edge of S = 1
    for nnz in range(1700, 1900):
        assert lib_plan(300, 606, nnz, 7, 4) == (OK,) + model_plan(300, 606, nnz, 7, 4)
    assert {p[:2] for p in seen} >= {(2, S) for S in (64, 32, 16, 8, 4, 2, 1)} | {(3, 0)}
    assert {p[2] for p in seen} == {0, 76, 156} and {p[3:] for p in seen} >= {(8, 4), (32, 16), (32, 4), (8, 16)}
    # node kernel -> unlimited kernel by size: the first (3,6) n whose syndrome bytes pass 156 KiB less 1024
    n = 6
    while node_lds_bytes((n + 6) // 2, n + 6) + 1024 <= KIB156:
        n += 6
    assert 23000 < n < 24000
    assert lib_plan(*regular(n))[1:] == (3, 0, node_lds_bytes(n // 2, n), 0, 8, 4)
    assert lib_plan(*regular(n + 6))[1:] == (5, 0, 0, 0, 0, 0)
    # the uint16 graph copies: a graph that is small in bytes never exists at 65535, so only the rule is held here
    assert lib_plan(10, 65535, 0, 0, 0)[1] != 2 and lib_plan(65535, 10, 0, 0, 0)[1] != 2 and lib_plan(10, 10, 0, 0, 0)[1:3] == (2, 64)


def test_degree_buckets_wide_graphs_and_forced_kernels():
    s, n, nnz = 60, 120, 360
    for cdeg, DC in ((0, 8), (1, 8), (8, 8), (9, 32), (32, 32)):
        for bdeg, DV in ((0, 4), (4, 4), (5, 16), (16, 16)):
            assert lib_plan(s, n, nnz, cdeg, bdeg)[1:] == (2, 8, lds_bytes(s, n, nnz, 8), 76, DC, DV)
            assert lib_plan(s, n, nnz, cdeg, bdeg, 1)[1:] == (3, 0, node_lds_bytes(s, n), 0, DC, DV)
            assert lib_plan(s, n, nnz, cdeg, bdeg, 2)[1:] == (5, 0, 0, 0, 0, 0)
            assert lib_plan(s, n, nnz, cdeg, bdeg, 7)[1:] == (5, 0, 0, 0, 0, 0)
    # wide graphs answer the unlimited kernel whatever their size and whatever is forced
    for sz in ((3, 5, 0), (12, 40, 60), (60, 120, 360), (4000, 8000, 24000), (30000, 60000, 180000)):
        for cdeg, bdeg in ((33, 3), (6, 17), (33, 17), (40, 20), (1000, 1)):
            for force in (0, 1, 2):
                assert lib_plan(*sz, cdeg, bdeg, force) == (OK, 5, 0, 0, 0, 0, 0), (sz, cdeg, bdeg, force)
        assert lib_plan(*sz, 32, 16)[1] == model_plan(*sz, 32, 16)[0] and (lib_plan(*sz, 32, 16)[1] in (2, 3) or sz[1] > 20000)


@pytest.mark.parametrize("experiments", [False, True])
def test_refusals_and_null_outputs(experiments):
    L = ldpc._capi.lib(experiments)
    for bad in ((-1, 10, 10, 3, 3, 0), (10, -1, 10, 3, 3, 0), (10, 10, -1, 3, 3, 0), (10, 10, 10, -1, 3, 0), (10, 10, 10, 3, -1, 0),
                (10, 10, 10, 3, 3, -1)):
        assert lib_plan(*bad, experiments=experiments) == (INVALID,)
        assert b"negative" in L.ldpc_last_error()
    top = 1 << 28
    for big in ((top, 10, 10), (10, top, 10), (10, 10, top), (1 << 40, 1 << 40, 1 << 40)):
        assert lib_plan(*big, 3, 3, experiments=experiments) == (UNSUPPORTED,)
        assert b"too large" in L.ldpc_last_error()
    assert lib_plan(top - 1, top - 1, top - 1, 3, 3, experiments=experiments)[:2] == (OK, 5)
    assert L.ldpc_debug_bpots_plan(60, 120, 360, 6, 3, 0, None, None, None, None, None, None) == OK   # every out pointer may be NULL
    assert L.ldpc_debug_bpots_last_launch(None, None, None, None, None, None) == INVALID
    for name in ("ldpc_debug_bpots_plan", "ldpc_debug_bpots_last_launch"):
        assert name in ldpc._capi.DEBUG_SYMBOLS


def test_bpots_plan_under_sanitizers(tmp_path):
    """csrc/bpots_plan.hpp built with a plain C++ compiler (it includes no HIP) under AddressSanitizer + UBSan, CPU only, and
    driven by tests/native/bpots_plan_sanitize.cpp."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "bpots_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *san, "-I", os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "bpots_plan_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK ") and "bpots plans" in out.stdout, out.stdout + out.stderr
