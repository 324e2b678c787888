"""Bit-packed (Julia BitMatrix layout) entries on the GPU.  Every comparison is exact.  The yardsticks are the byte
entry ldpc_bp_decode_batch on the whole batch (the same kernels under the same plan: hard decisions, flags, iteration
counts and LLRs must be the same bits) and the CPU oracle on a sample -- never the bits entry against itself."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import BPOracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = [0, 1, 63, 64, 777]
BATCHES = [1, 63, 64, 65, 1000]


def _bits(words):
    return np.unpackbits(words.view(np.uint8), bitorder="little")


def _words_with(flat_bits, bit0, rng, tail_words=3):
    """A word vector of seeded random bits whose bits [bit0, bit0 + len) are `flat_bits`."""
    nwords = (bit0 + flat_bits.size + 63) // 64 + tail_words
    words = rng.integers(0, 2 ** 63, nwords, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, nwords).astype(np.uint64)
    b = _bits(words)
    b[bit0:bit0 + flat_bits.size] = flat_bits
    return np.packbits(b, bitorder="little").view("<u8").copy()


def _irregular(n, s, seed):
    """Bits of degree 2..4 on random checks: odd n and s, check degrees all over the place."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j in range(n):
        for r in rng.choice(s, size=int(rng.integers(2, 5)), replace=False):
            rows.append(int(r)); cols.append(j)
    H = sp.csc_matrix((np.ones(len(rows), dtype=np.uint8), (rows, cols)), shape=(s, n))
    H.sort_indices()
    return H


def _syndromes(ldpc, H, B, per, seed):
    return ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(H.shape[1], B, per, seed=seed))


def _oracle_sample(H, per, max_iters, syn_bs, ref, k):
    """The byte entry's result (the yardstick of the whole batch) against the CPU oracle on the first k syndromes."""
    err, conv, llr, its = ref
    M = sp.csc_matrix(H); M.sort_indices()
    k = min(k, syn_bs.shape[0], 256)
    oc = BPOracle(csc=(M.indptr, M.indices), shape=M.shape, per=per, max_iters=max_iters)
    oerr, oconv, ollr, oits = oc.batchdecode(syn_bs[:k], want_llr=True)
    assert np.array_equal(err[:k], oerr) and np.array_equal(conv[:k], oconv)
    if its is not None:
        assert np.array_equal(its[:k], oits)
    return oerr, oconv, ollr, oits


def _check_bits_entry(dec, syn_bs, sbit0, ebit0, want_llr, want_iters, seed, ref=None, oracle=None):
    """One call of the bits entry on word vectors pre-filled with a seeded random pattern: every bit outside
    [ebit0, ebit0 + B n) keeps the pattern, every bit inside is the byte entry's hard decision; flags, iteration counts
    and LLRs are the byte entry's.  `oracle` = (oerr, oconv, ollr, oits) of the leading syndromes: compared too."""
    B, n = syn_bs.shape[0], dec.n
    if ref is None:
        ref = dec.decode_batch_host(syn_bs, want_llr=want_llr, want_iters=want_iters)
    rerr, rconv, rllr, rits = ref
    rng = np.random.default_rng(seed)
    syn_w = _words_with(np.ascontiguousarray(syn_bs).reshape(-1), sbit0, rng)
    err_w = _words_with(np.zeros(0, dtype=np.uint8), ebit0 + B * n, rng)   # all pattern
    pattern = _bits(err_w).copy()
    syn_before = syn_w.copy()
    conv, llr, its = dec.decode_batch_bits_words(B, syn_w, sbit0, err_w, ebit0, want_llr=want_llr, want_iters=want_iters)
    got = _bits(err_w)
    inside = got[ebit0:ebit0 + B * n].reshape(B, n)
    bad = np.nonzero(np.concatenate([got[:ebit0], got[ebit0 + B * n:]]) != np.concatenate([pattern[:ebit0], pattern[ebit0 + B * n:]]))[0]
    assert bad.size == 0, f"{bad.size} guard bits changed (first at index {bad[:5]} of the outside bits), offsets ({sbit0}, {ebit0})"
    assert np.array_equal(inside, rerr), f"hard decisions differ from the byte entry in columns {np.unique(np.nonzero(inside != rerr)[0])[:8]}, offsets ({sbit0}, {ebit0})"
    assert np.array_equal(conv, rconv)
    assert np.array_equal(syn_w, syn_before), "the syndrome words were written"
    if want_iters:
        assert np.array_equal(its, rits)
    else:
        assert its is None
    if want_llr:
        assert np.array_equal(llr.view(np.uint64), rllr.view(np.uint64)) or np.array_equal(llr, rllr, equal_nan=True)
    else:
        assert llr is None
    if oracle is not None:
        oerr, oconv, _, oits = oracle
        k = oerr.shape[0]
        assert np.array_equal(inside[:k], oerr) and np.array_equal(conv[:k], oconv)
        if want_iters:
            assert np.array_equal(its[:k], oits)
    return ref


FAMILIES = {
    # name: (code, per, max_iters, kernel_variant, kernel expected, batch from which on it is expected, oracle sample)
    "lds": (lambda ldpc: ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 30, 0, 2, 1, 64),
    "node": (lambda ldpc: ldpc.codes.parity_check_csc(4096, 8, 4), 0.03, 30, 0, 3, 1, 32),
    "team": (lambda ldpc: ldpc.codes.parity_check_csc(16384, 8, 4), 0.05, 12, 4, 4, 640, 16),
    "streaming": (lambda ldpc: ldpc.codes.parity_check_csc(16384, 8, 4), 0.05, 12, 1, 1, 1, 16),
    "streaming_second_pass": (lambda ldpc: ldpc.codes.parity_check_csc(4096, 8, 4), 0.065, 40, 1, 1, 1, 32),
    "irregular": (lambda ldpc: _irregular(1003, 517, 5), 0.02, 25, 0, None, 1, 64),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_family_through_the_bits_entry(ldpc, gpu, family):
    """One code per kernel family, batches 1, 63, 64, 65, 1000 (ragged last tile), offsets inside words: the bits entry
    equals the byte entry bit for bit, and both equal the oracle on a sample."""
    make, per, max_iters, variant, kernel, from_batch, k = FAMILIES[family]
    H = make(ldpc)
    dec = ldpc.BeliefPropagationDecoder(H, per, max_iters, kernel_variant=variant)
    for B in BATCHES + ([640] if family == "team" else []):
        syn = _syndromes(ldpc, H, B, per, seed=B + 17)
        ref = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
        oracle = _oracle_sample(H, per, max_iters, syn, ref, k)
        _check_bits_entry(dec, syn, 777, 63, True, True, seed=B, ref=ref, oracle=oracle)
        if kernel is not None and B >= from_batch:
            assert dec.info().last_kernel == kernel, (family, B, dec.info().last_kernel)
        _check_bits_entry(dec, syn, 0, 0, False, False, seed=B + 1, oracle=oracle)
    if family == "streaming_second_pass":
        assert 0 < int(ref[1].sum()) < 1000, "the waterfall batch should be mixed (stragglers for the second pass)"
    dec.close()


@pytest.mark.parametrize("make,per,max_iters", [
    (lambda ldpc: ldpc.codes.parity_check_csc(1000, 10, 9), 0.01, 30),
    (lambda ldpc: _irregular(1003, 517, 6), 0.02, 25),
], ids=["n1000_s900", "n1003_s517"])
def test_bit_offsets_and_guard_bits(ldpc, gpu, make, per, max_iters):
    """syndrome_bit0 and error_bit0 in {0, 1, 63, 64, 777}, independently (25 pairs), batch 65 (B n and B s are no
    multiples of 64): every bit outside the error range keeps the seeded pattern, every bit inside is the byte entry's."""
    H = make(ldpc)
    dec = ldpc.BeliefPropagationDecoder(H, per, max_iters)
    syn = _syndromes(ldpc, H, 65, per, seed=99)
    ref = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
    oracle = _oracle_sample(H, per, max_iters, syn, ref, 65)
    for sbit0 in OFFSETS:
        for ebit0 in OFFSETS:
            _check_bits_entry(dec, syn, sbit0, ebit0, True, True, seed=1000 * sbit0 + ebit0, ref=ref, oracle=oracle)
    dec.close()


def test_edge_inputs_and_optional_outputs(ldpc, gpu):
    """max_iters = 0 (the range becomes zeros, guard bits stay); per = 0 and per = 1 (non-finite LLRs, compared with
    equal_nan); llr / iters requested and not; one handle used alternately through the byte and the bits entry, twice each;
    batch 0 touches nothing."""
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    syn = _syndromes(ldpc, H, 130, 0.01, seed=4)
    dec0 = ldpc.BeliefPropagationDecoder(H, 0.01, 0)
    ref = _check_bits_entry(dec0, syn, 1, 777, True, True, seed=1)
    assert not ref[0].any() and not ref[1].any() and not ref[2].any() and not ref[3].any()
    dec0.close()
    for per in (0.0, 1.0):
        dec = ldpc.BeliefPropagationDecoder(H, per, 10)
        ref = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
        oracle = _oracle_sample(H, per, 10, syn, ref, 32)
        _check_bits_entry(dec, syn, 63, 1, True, True, seed=2, ref=ref, oracle=oracle)
        dec.close()
    dec = ldpc.BeliefPropagationDecoder(H, 0.01, 30)
    words = np.full(4, 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    conv, llr, its = dec.decode_batch_bits_words(0, words, 5, words, 7)
    assert conv.size == 0 and np.all(words == np.uint64(0xDEADBEEFCAFEF00D))
    ref = None
    for rep in range(2):                                        # byte, bits, byte, bits on one handle
        for want_llr in (False, True):
            for want_iters in (False, True):
                now = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
                if ref is not None:
                    assert all(np.array_equal(a, b) for a, b in zip(now, ref))
                ref = now
                _check_bits_entry(dec, syn, 64, 1, want_llr, want_iters, seed=rep, ref=ref)
    _oracle_sample(H, 0.01, 30, syn, ref, 64)
    assert dec.info().workspace_bytes >= 130 * 1900      # the byte staging is counted
    dec.close()
    with pytest.raises(IndexError):
        ldpc.BeliefPropagationDecoder(H, 0.01, 3).decode_batch_bits_words(2, np.zeros(28, np.uint64), 0, np.zeros(32, np.uint64), 0)   # 1792 < 2 * 900 bits


def test_host_pipeline_over_several_chunks(ldpc, gpu, monkeypatch):
    """A batch that goes through >= 3 chunks of the bits entry's host pipeline on a code with odd n and s: chunk borders
    fall inside words on both sides.  Equal to the byte entry column for column; LLRs and iteration counts too."""
    monkeypatch.setenv("LDPC_BITS_CHUNK_SYNDROMES", "9999")   # (read by the experiments build only)
    H = _irregular(1003, 517, 7)
    B = 40003                                                 # 5 chunks, the last one ragged; 5 MB of error bits
    syn = _syndromes(ldpc, H, B, 0.02, seed=8)
    dec = ldpc.BeliefPropagationDecoder(H, 0.02, 25, experiments=True)
    ref = dec.decode_batch_host(syn, want_llr=False, want_iters=True)
    oracle = _oracle_sample(H, 0.02, 25, syn, ref, 64)
    _check_bits_entry(dec, syn, 63, 777, False, True, seed=3, ref=ref, oracle=oracle)
    small = syn[:12001]                                       # 2 chunks with LLRs
    _check_bits_entry(dec, small, 1, 1, True, True, seed=4)
    dec.close()
    monkeypatch.delenv("LDPC_BITS_CHUNK_SYNDROMES")
    dec = ldpc.BeliefPropagationDecoder(H, 0.02, 25)          # the product build: one chunk through the same pipeline
    _check_bits_entry(dec, syn, 777, 1, False, True, seed=5, ref=ref, oracle=oracle)
    dec.close()


def _image_bytes(rows, syn_bytes, err_bytes, llr_bytes):
    """Bytes of a staging image [syndromes][errors][converged][iterations][LLRs] of `rows` syndromes, restated from
    csrc/host_pipe_plan.hpp stage_layout(): every region starts on a 256-byte boundary."""
    return sum((b + 255) // 256 * 256 for b in (syn_bytes, err_bytes, rows, 4 * rows, llr_bytes))


def test_pinned_ring_grows_slot_by_slot_on_one_handle(ldpc, gpu, monkeypatch):
    """The pinned ring of the host pipeline, shared by the byte and the bits entry, on ONE handle: a call of one chunk
    with a large image (only slot 0 is touched), then five chunks with a small image (slots 1 and 2 are allocated small),
    then three chunks with an image in between (slots 1 and 2 must grow: a single capacity for the whole ring would
    let the copies run past their end), all through the byte entry without LLRs; then the bits entry with four chunks
    whose image (LLRs) is larger than all of them.  Every result equals the device-resident entry column for column.
    (12001 syndromes of the n = 1003, s = 517 code: the bits entry's image without LLRs would be 2.3 MB and take the
    small-batch round trip, hence LLRs there.)"""
    import torch

    n, s, B = 1003, 517, 12001
    H = _irregular(n, s, 7)
    syn = _syndromes(ldpc, H, B, 0.02, seed=9)
    dec = ldpc.BeliefPropagationDecoder(H, 0.02, 25, experiments=True)
    d_err = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_conv = torch.empty(B, dtype=torch.uint8, device="cuda")
    d_it = torch.empty(B, dtype=torch.int32, device="cuda")
    d_llr = torch.empty((B, n), dtype=torch.float64, device="cuda")
    dec.decode_batch_device(torch.from_numpy(syn).cuda(), d_err, d_conv, d_llr, d_it)
    torch.cuda.synchronize()
    ref = (d_err.cpu().numpy(), d_conv.cpu().numpy(), d_llr.cpu().numpy(), d_it.cpu().numpy())
    assert 0 < int(ref[1].sum()) and ref[0].any()

    def byte_image(rows):
        return _image_bytes(rows, rows * s, rows * n, 0)

    def bits_image(rows):
        return _image_bytes(rows, ((rows * s + 63) // 64 + 1) * 8, ((rows * n + 63) // 64 + 1) * 8, 8 * rows * n)

    small_batch_limit = 4 << 20                               # whole-batch images up to this take the round trip instead
    assert byte_image(B) > small_batch_limit and bits_image(B) > small_batch_limit
    assert byte_image(3000) < byte_image(5000) < byte_image(12001) < bits_image(4000)
    for chunk, nchunks in ((12001, 1), (3000, 5), (5000, 3)):
        assert -(-B // chunk) == nchunks
        monkeypatch.setenv("LDPC_BITS_CHUNK_SYNDROMES", str(chunk))   # (the experiments build: both entries' chunk)
        err, conv, _, its = dec.decode_batch_host(syn, want_llr=False, want_iters=True)
        assert np.array_equal(err, ref[0]), f"chunk {chunk}: hard decisions differ in columns {np.unique(np.nonzero(err != ref[0])[0])[:8]}"
        assert np.array_equal(conv, ref[1]) and np.array_equal(its, ref[3]), f"chunk {chunk}"
    monkeypatch.setenv("LDPC_BITS_CHUNK_SYNDROMES", "4000")           # 4 chunks, the last one a single syndrome
    _check_bits_entry(dec, syn, 63, 777, True, True, seed=6, ref=ref)
    dec.close()


def test_device_form_on_a_side_stream(ldpc, gpu):
    """ldpc_bp_decode_batch_bits_device on torch tensors, on a non-default stream, two calls back to back without a
    synchronise in between; last_status() clean, last_timing() returns (total_ms spans the conversions)."""
    import torch

    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    dec = ldpc.BeliefPropagationDecoder(H, 0.01, 30, device=0)
    dev = torch.device("cuda:0")
    B, n, s = 1000, 1000, 900
    rng = np.random.default_rng(11)
    calls = []
    for i, (sbit0, ebit0) in enumerate([(63, 777), (1, 64)]):
        syn = _syndromes(ldpc, H, B, 0.01, seed=30 + i)
        ref = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
        _oracle_sample(H, 0.01, 30, syn, ref, 64)
        syn_w = _words_with(syn.reshape(-1), sbit0, rng)
        err_w = _words_with(np.zeros(0, dtype=np.uint8), ebit0 + B * n, rng)
        calls.append((sbit0, ebit0, ref, err_w,
                      torch.from_numpy(syn_w.view(np.int64)).to(dev), torch.from_numpy(err_w.view(np.int64)).to(dev),
                      torch.empty(B, dtype=torch.uint8, device=dev), torch.empty((B, n), dtype=torch.float64, device=dev),
                      torch.empty(B, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for sbit0, ebit0, _, _, d_syn, d_err, d_conv, d_llr, d_it in calls:      # no synchronise in between
            dec.decode_batch_bits_device(B, d_syn, sbit0, d_err, ebit0, d_conv, llr=d_llr, iters=d_it)
    dec.last_status()
    sweep_ms, total_ms, sum_iters = dec.last_timing()
    sweep1, total1, _ = dec.last_timing(1)
    side.synchronize()
    assert total_ms > 0 and total_ms >= sweep_ms > 0 and total1 >= sweep1 > 0
    for sbit0, ebit0, ref, pattern_w, _, d_err, d_conv, d_llr, d_it in calls:
        got, pattern = _bits(d_err.cpu().numpy().view(np.uint64)), _bits(pattern_w)
        assert np.array_equal(got[ebit0:ebit0 + B * n].reshape(B, n), ref[0])
        assert np.array_equal(got[:ebit0], pattern[:ebit0]) and np.array_equal(got[ebit0 + B * n:], pattern[ebit0 + B * n:])
        assert np.array_equal(d_conv.cpu().numpy(), ref[1]) and np.array_equal(d_it.cpu().numpy(), ref[3])
        assert np.array_equal(d_llr.cpu().numpy().view(np.uint64), ref[2].view(np.uint64))
    assert sum_iters == int(calls[1][2][3].sum())
    dec.close()
    multi = ldpc.BeliefPropagationDecoder(H, 0.01, 30, devices=[0, 0])
    with pytest.raises(ldpc.LdpcError) as ei:
        multi.decode_batch_bits_device(B, calls[0][4], 0, calls[0][5], 0, calls[0][6])
    assert ei.value.status == 5
    multi.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_host_form_shares_words_between_shards(ldpc, gpu, devices):
    """ldpc_bp_decode_batch_multi_bits with logical devices on GPU 0: n = 1003 and batch 1001 put every shard border
    inside a word.  Equal to the byte entry of a single-device decoder and to the oracle sample; guard bits intact."""
    H = _irregular(1003, 517, 9)
    B = 1001
    syn = _syndromes(ldpc, H, B, 0.02, seed=12)
    single = ldpc.BeliefPropagationDecoder(H, 0.02, 25, device=0)
    ref = single.decode_batch_host(syn, want_llr=True, want_iters=True)
    oracle = _oracle_sample(H, 0.02, 25, syn, ref, 64)
    single.close()
    G = len(devices)
    for g in range(1, G):
        assert ((g * B // G) * 1003 + 63) % 64 != 0, "shard border on a word border: pick another batch"
    multi = ldpc.BeliefPropagationDecoder(H, 0.02, 25, devices=devices)
    for sbit0, ebit0 in [(0, 0), (63, 63), (777, 1)]:
        _check_bits_entry(multi, syn, sbit0, ebit0, True, True, seed=sbit0 + G, ref=ref, oracle=oracle)
    tiny = syn[:2]                                            # fewer columns than devices: empty shards
    _check_bits_entry(multi, tiny, 1, 1, False, False, seed=5, ref=tuple(a[:2] if a is not None else None for a in (ref[0], ref[1], None, None)))
    multi.close()


def test_batchdecode_with_bitmatrices(ldpc, gpu):
    """batchdecode_ with (BitMatrix, BitMatrix), (dense, BitMatrix) -- the reference doctest's shape -- and the
    unchanged (dense, dense): the same errors / success; the scratch holds the last column as before."""
    H = ldpc.parity_check_matrix(1000, 10, 9)
    dec = ldpc.BeliefPropagationDecoder(H, 0.01, 100)
    B = 77
    e = ldpc.codes.random_errors(1000, B, 0.01, seed=21)
    syn_bs = ldpc.codes.syndromes_of(H, e)
    S = np.asfortranarray(syn_bs.T.astype(np.int64))          # s x B, like (H * errors) .% 2
    dense_err = np.zeros((1000, B), dtype=np.uint8)
    _, ok_dense = ldpc.batchdecode_(dec, S, dense_err)
    scratch_err, scratch_llr = dec.scratch.err.copy(), dec.scratch.log_probabs.copy()
    M = sp.csc_matrix(H); M.sort_indices()
    oc = BPOracle(csc=(M.indptr, M.indices), shape=M.shape, per=0.01, max_iters=100)
    oerr, oconv, ollr, _ = oc.batchdecode(syn_bs, want_llr=True)
    assert np.array_equal(dense_err.T, oerr) and np.array_equal(ok_dense, oconv.astype(bool))
    for syndromes in (ldpc.BitMatrix.from_dense(S), S):
        errors = ldpc.BitMatrix.zeros(1000, B)
        dec.scratch.err[:] = 7; dec.scratch.log_probabs[:] = 7
        got, ok = ldpc.batchdecode_(dec, syndromes, errors)
        assert got is errors and errors.trailing_bits_zero()
        assert np.array_equal(errors.to_dense(), dense_err) and np.array_equal(ok, ok_dense)
        assert np.array_equal(dec.scratch.err, scratch_err)
        assert np.array_equal(dec.scratch.log_probabs.view(np.uint64), scratch_llr.view(np.uint64))
    assert np.array_equal(scratch_err, dense_err[:, -1])
    fin = np.isfinite(ollr[-1])
    assert np.max(np.abs(scratch_llr[fin] - ollr[-1][fin])) <= 1e-5
    out2 = np.zeros((1000, B), dtype=np.float64)              # BitMatrix syndromes, dense errors
    _, ok2 = ldpc.batchdecode_(dec, ldpc.BitMatrix.from_dense(S), out2, np.zeros(B, dtype=np.bool_))
    assert np.array_equal(out2, dense_err) and np.array_equal(ok2, ok_dense)
    err_bm, conv, llr, its = dec.decode_batch_bits_host(ldpc.BitMatrix.from_dense(S), want_llr=True, want_iters=True)
    assert np.array_equal(err_bm.to_dense().T, oerr) and np.array_equal(conv, oconv)
    dec.close()


def test_c_host_decodes_through_the_bits_entry(tmp_path, gpu):
    """tests/abi_bits_driver.c "gpu": a plain-C host decodes through ldpc_bp_decode_batch_bits at offsets inside words
    and compares every bit, flag, count and LLR with ldpc_bp_decode_batch."""
    import ldpcdecoders_jl_amd as ldpc

    exe = str(tmp_path / "abi_bits_driver")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_bits_driver.c"), "-o", exe,
                           ldpc._capi.LIB_PATH, "-Wl,-rpath," + os.path.dirname(ldpc._capi.LIB_PATH),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "abi_bits_driver gpu ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
