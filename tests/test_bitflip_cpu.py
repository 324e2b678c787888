"""Bit-flip decoder without a GPU: the new C entries exist in both builds and validate their arguments before any
device work, the Python mirror fails loudly without a device, and the CPU model (tests/bitflip_model.py), the yardstick of
tests/test_gpu_bitflip.py, checks itself against the reference's definition."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ldpcdecoders_jl_amd as ldpc
from bitflip_model import GOLDEN, TIE_FIRST, TIE_LAST, TIE_RANDOM, BitFlipModel, chooser_for, mix, random_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldpc_bitflip_create", "ldpc_bitflip_destroy", "ldpc_bitflip_kernel", "ldpc_bitflip_decode_batch",
               "ldpc_bitflip_decode_batch_device")


@pytest.mark.parametrize("experiments", [False, True])
def test_new_symbols_are_exported_by_both_builds(experiments):
    lib = ldpc._capi.lib(experiments)
    for name in NEW_SYMBOLS:
        assert name in ldpc._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ldpc_abi_version() == 4   # added by symbol, like the bits entries


def _options(**kw):
    o = ldpc._capi.BitFlipOptions()
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_options_struct_layout():
    """int32 device, int32 tie_break, uint64 seed, int32 kernel_variant, int32 reserved[11] = 64 bytes, seed at 8."""
    assert ctypes.sizeof(ldpc._capi.BitFlipOptions) == 64
    assert ldpc._capi.BitFlipOptions.seed.offset == 8 and ldpc._capi.BitFlipOptions.kernel_variant.offset == 16


def test_argument_validation_happens_before_any_device_work():
    lib = ldpc._capi.lib()
    h = ctypes.c_void_p()
    colptr = np.array([0, 2, 2], dtype=np.int64)
    good = np.array([0, 1], dtype=np.int64)
    for bad, word in ((np.array([1, 0], dtype=np.int64), b"ascending"), (np.array([0, 5], dtype=np.int64), b"outside")):
        st = lib.ldpc_bitflip_create(2, 2, 2, colptr.ctypes.data, bad.ctypes.data, 0.1, 5, None, ctypes.byref(h))
        assert st == 1 and word in lib.ldpc_last_error() and not h.value
    assert lib.ldpc_bitflip_create(2, 2, 3, colptr.ctypes.data, good.ctypes.data, 0.1, 5, None, ctypes.byref(h)) == 1
    assert lib.ldpc_bitflip_create(2, 2, 2, colptr.ctypes.data, good.ctypes.data, 0.1, -1, None, ctypes.byref(h)) == 1
    assert lib.ldpc_bitflip_create(2, 2, 2, colptr.ctypes.data, good.ctypes.data, 0.1, 5, None, None) == 1
    for tie in (-1, 3):
        o = _options(tie_break=tie)
        st = lib.ldpc_bitflip_create(2, 2, 2, colptr.ctypes.data, good.ctypes.data, 0.1, 5, ctypes.byref(o), ctypes.byref(h))
        assert st == 1 and b"tie_break" in lib.ldpc_last_error() and not h.value
    o = _options(kernel_variant=9)
    assert lib.ldpc_bitflip_create(2, 2, 2, colptr.ctypes.data, good.ctypes.data, 0.1, 5, ctypes.byref(o), ctypes.byref(h)) == 1
    # NULL handle / negative column0 at the batch entries
    buf = np.zeros(8, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.ldpc_bitflip_decode_batch(None, 1, 0, p, p, p, None, None) == 1
    assert lib.ldpc_bitflip_decode_batch(None, 1, -1, p, p, p, None, None) == 1
    assert lib.ldpc_bitflip_decode_batch_device(None, 1, 0, None, None, None, None, None, None) == 1
    assert lib.ldpc_bitflip_destroy(None) == 0 and lib.ldpc_bitflip_kernel(None) == 0


def test_no_cpu_fallback_and_the_package_does_not_import_the_model():
    lib = ldpc._capi.lib()
    if lib.ldpc_device_count() == 0:
        with pytest.raises(ldpc.LdpcError) as ei:
            ldpc.BitFlipDecoder(ldpc.parity_check_matrix(96, 6, 3), 0.01, 10)
        assert ei.value.status == 2
    with pytest.raises(TypeError):
        ldpc.BitFlipDecoder(ldpc.parity_check_matrix(96, 6, 3), 1, 10)      # per::Float64
    with pytest.raises(TypeError):
        ldpc.BitFlipDecoder(ldpc.parity_check_matrix(96, 6, 3), 0.1, 10.0)  # max_iters::Int
    pkg = os.path.join(ROOT, "ldpcdecoders.jl_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".jl")):
                assert "bitflip_model" not in open(os.path.join(dp, f), errors="replace").read(), f


def test_mix_is_the_splitmix64_finaliser():
    """Three values computed by hand from the header's five lines; they are also the first three outputs of the
    published SplitMix64 generator seeded with 0 (whose state advances by the golden-ratio constant)."""
    assert GOLDEN == 0x9E3779B97F4A7C15
    assert mix(GOLDEN) == 0xE220A8397B1DCDAF
    assert mix(2 * GOLDEN) == 0x6E789E6AA1B965F4
    assert mix(3 * GOLDEN) == 0x06C45D188009454F
    assert mix(0) == 0
    # the rank is the upper half of r scaled to [0, k): in range, and a function of (seed, column, iteration) only
    for k in (1, 2, 11, 1000):
        ranks = {random_rank(5, c, it, k) for c in range(40) for it in range(1, 6)}
        assert min(ranks) >= 0 and max(ranks) < k and (k == 1 or len(ranks) > 1)
    r = mix(mix(7 + GOLDEN * 4) + 2)
    assert random_rank(7, 3, 2, 11) == ((r >> 32) * 11) >> 32


def _reference_votes(H, syndrome, flips_so_far_per_iteration):
    """The votes the reference holds in iteration len(flips) + 1, from its definition alone (dense, no model code):
    sum over the executed iterations of (+1 per mismatched, -1 per matched check of the bit)."""
    Hd = np.asarray(sp.csr_matrix(H).todense()).astype(np.int64)
    err = np.zeros(Hd.shape[1], dtype=np.int64)
    votes = np.zeros(Hd.shape[1], dtype=np.int64)
    out = []
    for j in list(flips_so_far_per_iteration) + [None]:
        mism = ((Hd @ err) % 2) != syndrome
        votes = votes + Hd.T @ np.where(mism, 1, -1)
        out.append(votes.copy())
        if j is not None:
            err[j] ^= 1
    return out


@pytest.mark.parametrize("tie", [TIE_RANDOM, TIE_FIRST, TIE_LAST])
def test_every_chosen_index_is_a_maximiser_of_the_reference_votes(tie):
    """So any model output is one the reference produces for some realisation of its rand calls."""
    H = ldpc.codes.parity_check_csc(200, 10, 9)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(200, 6, 0.03, seed=3))
    m = BitFlipModel(H, 40)
    ties = 0
    for c in range(6):
        trace = []
        m.decode(syn[c], chooser_for(tie, seed=11), column=c, trace=trace)
        assert trace
        ref = _reference_votes(H, syn[c].astype(np.int64), [t[3] for t in trace])
        for (it, votes, cand, j), rv in zip(trace, ref):
            assert np.array_equal(votes, rv), (c, it)
            assert rv[j] == rv.max() and rv.max() >= 0
            assert np.array_equal(cand, np.nonzero(rv == rv.max())[0])
            ties += len(cand) > 1
    assert ties > 0   # the input exercises the tie rule


def test_model_on_hand_checked_cases():
    H3 = np.ones((3, 3), dtype=np.bool_)
    m = BitFlipModel(H3, 10)
    # every vote is +1 - 1 - 1 = -1: no bit with a non-negative vote
    err, conv, its, stop = m.decode(np.array([1, 0, 0]), chooser_for(TIE_FIRST))
    assert not err.any() and conv is True and its == 1 and stop == 2
    # all-zero syndrome: matched in the first iteration
    err, conv, its, stop = m.decode(np.zeros(3, dtype=np.int64), chooser_for(TIE_RANDOM))
    assert not err.any() and conv and its == 1 and stop == 1
    # max_iters = 0: zeros, false
    err, conv, its, stop = BitFlipModel(H3, 0).decode(np.array([1, 1, 1]), chooser_for(TIE_LAST))
    assert not err.any() and conv is False and its == 0 and stop == 0
    # syndrome (1, 1, 1): every vote +3, FIRST flips bit 0, LAST bit 2; matched in iteration 2
    for tie, bit in ((TIE_FIRST, 0), (TIE_LAST, 2)):
        err, conv, its, stop = m.decode(np.array([1, 1, 1]), chooser_for(tie))
        assert err.tolist() == [int(j == bit) for j in range(3)] and conv and its == 2 and stop == 1
    # an entry other than 0/1 never matches: votes 3, 2, 5, 4, ... (check 0 always adds +1), bit 0 is toggled ten times
    err, conv, its, stop = m.decode(np.array([2, 1, 1]), chooser_for(TIE_FIRST))
    assert not err.any() and conv is False and its == 10 and stop == 0
    # stored zeros are not edges
    Hz = sp.csc_matrix((np.array([1, 0, 1, 1], dtype=np.uint8), np.array([0, 1, 1, 0]), np.array([0, 2, 3, 4])), shape=(2, 3))
    assert BitFlipModel(Hz, 1).H.nnz == 3


def _build_driver(tmp_path):
    exe = str(tmp_path / "abi_bitflip_driver")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_bitflip_driver.c"), "-o", exe,
                           ldpc._capi.LIB_PATH, "-Wl,-rpath," + os.path.dirname(ldpc._capi.LIB_PATH),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_bitflip_entries_link_and_validate_from_a_c_host(tmp_path):
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
