"""The layers of the layered min-sum schedule without a GPU: ldpc_debug_layer_plan (csrc/layer_plan.cpp, what
ldpc_minsum_create uploads) against the first fit of the numpy model (tests/layered_model.py), the property the kernel
relies on -- no two checks of a layer share a bit -- asserted directly, the layer counts, and the planner under the
sanitizers on the same graphs."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from layered_model import layers_of
from test_gpu_minsum import _irregular

INVALID = 1


def _pattern(H):
    M = sp.csc_matrix(H)
    M = sp.csc_matrix((np.ones(M.nnz, dtype=np.uint8), M.indices, M.indptr), shape=M.shape)
    M.sort_indices()
    return M


def graphs(ldpc):
    """name -> (pattern, K or None)."""
    Hx, Hz = ldpc.codes.bivariate_bicycle_72_12_6()
    every = np.zeros((6, 40), dtype=np.uint8)           # row 2 touches every bit: a layer of its own
    for i, lo in ((0, 0), (1, 10), (3, 20), (4, 30), (5, 5)):
        every[i, lo:lo + 10] = 1
    every[2, :] = 1
    return {
        "bb72_hx": (_pattern(np.asarray(Hx, dtype=np.uint8)), 4),
        "bb72_hz": (_pattern(np.asarray(Hz, dtype=np.uint8)), None),
        "240_8_4": (_pattern(ldpc.parity_check_matrix(240, 8, 4)), 4),
        "1000_10_9": (_pattern(ldpc.parity_check_matrix(1000, 10, 9)), 9),
        "irregular": (_pattern(_irregular()[0]), None),
        "one_row_every_bit": (_pattern(every), None),
        "no_edges": (_pattern(np.zeros((5, 7), dtype=np.uint8)), 0),
    }


def library_layers(ldpc, M, experiments=False):
    lib = ldpc._capi.lib(experiments)
    s, n = M.shape
    colptr, rowval = M.indptr.astype(np.int64), np.append(M.indices.astype(np.int64), 0)   # (never empty: a pointer to hand over)
    layer_of = np.full(s, -7, dtype=np.int32)
    K = ctypes.c_int32(-7)
    st = lib.ldpc_debug_layer_plan(s, n, colptr.ctypes.data, rowval.ctypes.data, layer_of.ctypes.data, ctypes.byref(K))
    assert st == 0, lib.ldpc_last_error().decode()
    return layer_of, K.value


def assert_disjoint(M, layer_of, K):
    """Per layer the bit sets of its checks are pairwise disjoint; every non-empty check has a layer, an empty one none."""
    R = sp.csr_matrix(M)
    deg = np.diff(R.indptr)
    assert np.array_equal(layer_of >= 0, deg > 0) and np.all(layer_of[deg == 0] == -1)
    assert (layer_of.max(initial=-1) + 1) == K
    for k in range(K):
        rows = np.nonzero(layer_of == k)[0]
        assert rows.size > 0                                                # first fit leaves no layer empty
        per_bit = np.asarray(R[rows].sum(axis=0)).ravel()
        assert per_bit.max(initial=0) <= 1, f"layer {k}: a bit in two checks"


@pytest.mark.parametrize("name", ["bb72_hx", "bb72_hz", "240_8_4", "1000_10_9", "irregular", "one_row_every_bit", "no_edges"])
def test_library_layers_equal_the_first_fit_of_the_model(ldpc, name):
    M, K_known = graphs(ldpc)[name]
    want, K_model = layers_of(M)
    for experiments in (False, True):
        got, K = library_layers(ldpc, M, experiments)
        assert K == K_model and np.array_equal(got, want), (name, K, K_model)
        assert_disjoint(M, got, K)
    if K_known is not None:
        assert K == K_known
    if name == "one_row_every_bit":
        assert (got == got[2]).sum() == 1 and K == 3                         # rows 0 and 5 meet in bits 5 .. 9
    if name == "irregular":
        deg = np.diff(sp.csr_matrix(M).indptr)
        assert got[0] == -1 and deg[0] == 0                                  # the empty check
        assert got[1:5].tolist() == [0, 0, 1, 0]                             # bits 5 | 10..42 | 20..83 | 60..129: only 3 meets 2 (and 4)
    if name == "no_edges":
        assert np.all(got == -1)


def test_gallager_codes_get_one_layer_per_block(ldpc):
    """parity_check_matrix stacks wc blocks of n / wr checks, each block a permutation of the first: first fit puts block
    b into layer b only if every check of block b meets some check of each earlier block -- true for these two codes."""
    for n, wr, wc in ((240, 8, 4), (1000, 10, 9)):
        got, K = library_layers(ldpc, _pattern(ldpc.parity_check_matrix(n, wr, wc)))
        assert K == wc and np.array_equal(got, np.repeat(np.arange(wc), n // wr))


def test_refusals_and_optional_outputs(ldpc):
    lib = ldpc._capi.lib()
    assert "ldpc_debug_layer_plan" in ldpc._capi.DEBUG_SYMBOLS and "ldpc_minsum_layers" in ldpc._capi.EXPORTED_SYMBOLS
    colptr = np.array([0, 2, 2], dtype=np.int64)
    K = ctypes.c_int32(-7)
    for rowval, word in ((np.array([1, 0], dtype=np.int64), "ascending"), (np.array([0, 5], dtype=np.int64), "outside")):
        assert lib.ldpc_debug_layer_plan(2, 2, colptr.ctypes.data, rowval.ctypes.data, None, ctypes.byref(K)) == INVALID
        assert word in lib.ldpc_last_error().decode() and K.value == -7
    assert lib.ldpc_debug_layer_plan(2, 2, None, None, None, None) == INVALID
    assert lib.ldpc_debug_layer_plan(-1, 2, colptr.ctypes.data, colptr.ctypes.data, None, None) == INVALID
    good = np.array([0, 1], dtype=np.int64)
    assert lib.ldpc_debug_layer_plan(2, 2, colptr.ctypes.data, good.ctypes.data, None, ctypes.byref(K)) == 0 and K.value == 2
    layer_of = np.full(2, -7, dtype=np.int32)
    assert lib.ldpc_debug_layer_plan(2, 2, colptr.ctypes.data, good.ctypes.data, layer_of.ctypes.data, None) == 0
    assert layer_of.tolist() == [0, 1]                                       # both checks hold bit 0
    assert lib.ldpc_minsum_layers(None) == 0


def test_layer_plan_under_sanitizers(ldpc, tmp_path):
    """layer_plan.cpp built with AddressSanitizer + UBSan (CPU only) and driven by tests/native/layer_plan_sanitize.cpp on
    the graphs above (handed over in a file, with the model's assignment) and on the inputs the planner and its
    verification refuse."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for name, (M, _) in graphs(ldpc).items():
        R = sp.csr_matrix(M)
        R.sort_indices()
        want, K = layers_of(M)
        lines.append(f"{R.shape[0]} {R.shape[1]} {R.nnz} {K}")
        for arr in (R.indptr, R.indices, want):
            lines.append(" ".join(str(int(v)) for v in arr))
    path = tmp_path / "graphs.txt"
    path.write_text("\n".join(lines) + "\n")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "layer_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", *san, "-o", exe, os.path.join(root, "tests", "native", "layer_plan_sanitize.cpp"),
                           os.path.join(root, "ldpcdecoders.jl_amd", "csrc", "layer_plan.cpp")])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK 7 graphs"), out.stdout + out.stderr
