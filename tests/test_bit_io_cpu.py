"""Bit-packed (Julia BitMatrix layout) batch entries, the part that needs no GPU: the host mirror of the layout, the
three new symbols of the C ABI and their argument checks (refused before any device work), and a plain-C consumer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ldpcdecoders_jl_amd as ldpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(67, 5), (64, 64), (1, 1), (1000, 3), (0, 4), (3, 0), (63, 1), (65, 63)]
BITS_SYMBOLS = ("ldpc_bp_decode_batch_bits", "ldpc_bp_decode_batch_bits_device", "ldpc_bp_decode_batch_multi_bits")


def _bit(chunks, k):
    return (int(chunks[k >> 6]) >> (k & 63)) & 1


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bitmatrix_layout_is_julias(rows, cols):
    """Element (r, c) is bit c * rows + r of the flat string: word k >> 6, bit k & 63, LSB first, columns not padded,
    trailing bits zero -- checked element by element against that formula, and against numpy's packbits."""
    rng = np.random.default_rng(rows * 131 + cols)
    X = rng.integers(0, 2, (rows, cols)).astype(np.uint8)
    b = ldpc.BitMatrix.from_dense(X)
    assert b.shape == (rows, cols) and b.chunks.dtype == np.uint64 and b.chunks.size == (rows * cols + 63) // 64
    for c in range(cols):
        for r in range(0, rows, max(1, rows // 97)):
            assert _bit(b.chunks, c * rows + r) == X[r, c], (r, c)
    for k in range(rows * cols, 64 * b.chunks.size):
        assert _bit(b.chunks, k) == 0, f"trailing bit {k} set"
    assert b.trailing_bits_zero()
    packed = np.packbits(X.ravel(order="F"), bitorder="little")
    want = np.zeros(8 * b.chunks.size, dtype=np.uint8)
    want[:packed.size] = packed
    assert np.array_equal(b.chunks, want.view("<u8"))
    assert np.array_equal(b.to_dense(), X) and b.to_dense().shape == (rows, cols)
    for c in range(min(cols, 3)):
        assert np.array_equal(b.column(c), X[:, c])
    assert ldpc.BitMatrix.from_dense(b.to_dense()) == b


def test_bitmatrix_zeros_columns_and_checks():
    z = ldpc.BitMatrix.zeros(67, 5)
    assert z.shape == (67, 5) and not z.chunks.any() and z.chunks.size == 6 and z.to_dense().sum() == 0
    chunks, bit0 = z.columns(2, 4)
    assert chunks is z.chunks and bit0 == 2 * 67
    assert z.columns(0, 5)[1] == 0 and z.columns(5, 5)[1] == 5 * 67
    with pytest.raises(IndexError):
        z.columns(3, 6)
    with pytest.raises(IndexError):
        z.columns(4, 3)
    with pytest.raises(ValueError):
        ldpc.BitMatrix(67, 5, np.zeros(5, dtype=np.uint64))
    with pytest.raises(ValueError):
        ldpc.BitMatrix(67, 5, np.zeros(6, dtype=np.int64))
    # non-zero of any element type is a set bit (Bool, Int, Float64 matrices)
    X = np.array([[0, 2], [1.5, 0], [-1, 0]])
    assert np.array_equal(ldpc.BitMatrix.from_dense(X).to_dense(), (X != 0).astype(np.uint8))


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"ldpc_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, f"{name} is not declared in include/ldpc_mi355x.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("experiments", [False, True])
def test_bits_symbols_are_exported_with_the_declared_signatures(experiments):
    lib = ldpc._capi.lib(experiments)
    host = ["ldpc_bp_decoder *dec", "int64_t batch", "const uint64_t *syndrome_words", "int64_t syndrome_bit0",
            "uint64_t *error_words", "int64_t error_bit0", "uint8_t *converged", "double *llr", "int32_t *iters"]
    assert _prototype("ldpc_bp_decode_batch_bits") == host
    assert _prototype("ldpc_bp_decode_batch_multi_bits") == ["ldpc_bp_multi *dec"] + host[1:]
    assert _prototype("ldpc_bp_decode_batch_bits_device") == [
        "ldpc_bp_decoder *dec", "int64_t batch", "const uint64_t *d_syndrome_words", "int64_t syndrome_bit0",
        "uint64_t *d_error_words", "int64_t error_bit0", "uint8_t *d_converged", "double *d_llr", "int32_t *d_iters",
        "void *stream"]
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for name in BITS_SYMBOLS:
        assert name in ldpc._capi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        nargs = 10 if name.endswith("_device") else 9
        assert fn.restype == ctypes.c_int32 and fn.argtypes == [vp, i64, vp, i64, vp, i64] + [vp] * (nargs - 6)
    assert lib.ldpc_abi_version() == 4   # the entries only add symbols: callers find them by symbol lookup


@pytest.mark.parametrize("experiments", [False, True])
@pytest.mark.parametrize("name", BITS_SYMBOLS)
def test_bits_entries_refuse_bad_arguments_without_a_device(name, experiments):
    """NULL handle, negative batch, negative bit offsets: LDPC_ERR_INVALID_ARGUMENT (1) before any device work."""
    lib = ldpc._capi.lib(experiments)
    fn = getattr(lib, name)
    tail = (None,) if name.endswith("_device") else ()
    words = np.zeros(4, dtype=np.uint64)
    conv = np.zeros(4, dtype=np.uint8)
    w, c = words.ctypes.data, conv.ctypes.data
    assert fn(None, 1, w, 0, w, 0, c, None, None, *tail) == 1
    assert b"NULL" in lib.ldpc_last_error()
    assert fn(None, 0, w, 0, w, 0, c, None, None, *tail) == 1
    assert fn(None, -1, w, 0, w, 0, c, None, None, *tail) == 1
    assert fn(None, 1, w, -1, w, 0, c, None, None, *tail) == 1
    assert fn(None, 1, w, 0, w, -1, c, None, None, *tail) == 1


def _build_bits_driver(tmp_path):
    exe = str(tmp_path / "abi_bits_driver")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_bits_driver.c"), "-o", exe,
                           ldpc._capi.LIB_PATH, "-Wl,-rpath," + os.path.dirname(ldpc._capi.LIB_PATH),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_host_compiles_links_and_checks_arguments(tmp_path):
    """tests/abi_bits_driver.c compiles as C99 with -Wall -Werror against the header, links against the library, and run
    without arguments exercises the argument checks of the three entries (exit status 0)."""
    exe = _build_bits_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "abi_bits_driver ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_batchdecode_keeps_rejecting_mismatched_bitmatrices():
    """Shape checks of batchdecode_ (belief_propagation.jl:221-222) hold for BitMatrix arguments, before any decoder
    work (a decoder object is not needed to see them)."""
    class Dummy(ldpc.AbstractDecoder):
        def decode_(self, syndrome):
            return np.zeros(4, dtype=np.uint8), True

    syn = ldpc.BitMatrix.zeros(3, 5)
    with pytest.raises(AssertionError):
        ldpc.batchdecode_(Dummy(), syn, ldpc.BitMatrix.zeros(4, 6))
    errs, ok = ldpc.batchdecode_(Dummy(), syn, ldpc.BitMatrix.zeros(4, 5))   # the generic per-column loop
    assert isinstance(errs, ldpc.BitMatrix) and ok.all() and errs.to_dense().sum() == 0
