"""Bit-flip decoder on the GPU.  Every comparison is against the CPU model (tests/bitflip_model.py: the reference's
loop restated, recomputing H * err and the votes in every iteration) and is exact in every element: there is no
floating point on the path, and the tie rule of include/ldpc_mi355x.h leaves one legal output."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from bitflip_model import TIE_FIRST, TIE_LAST, TIE_RANDOM, BitFlipModel, chooser_for, random_rank

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {"random": TIE_RANDOM, "first": TIE_FIRST, "last": TIE_LAST}


def _syndromes(ldpc, H, B, per, seed):
    e = ldpc.codes.random_errors(H.shape[1], B, per, seed=seed)
    return e, ldpc.codes.syndromes_of(H, e)


def _assert_equal_to_model(got, want, what=""):
    for name, g, w in zip(("errors", "converged", "iters", "stop_reason"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differ from the model in {bad.size} columns, first {bad[:8]}"


def _irregular(n, s, seed):
    """Bits of degree 2..4 on random checks, then bit 5 loses every edge (degree 0) and a new last check holds only bit 7
    (degree 1)."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j in range(n):
        if j == 5:
            continue
        for r in rng.choice(s - 1, size=int(rng.integers(2, 5)), replace=False):
            rows.append(int(r)); cols.append(j)
    rows.append(s - 1); cols.append(7)
    H = sp.csc_matrix((np.ones(len(rows), dtype=np.uint8), (rows, cols)), shape=(s, n))
    H.sort_indices()
    assert np.diff(H.indptr)[5] == 0 and np.diff(sp.csr_matrix(H).indptr)[s - 1] == 1
    return H


@pytest.mark.parametrize("per", [0.01, 0.03])
def test_reference_configuration_equals_the_model_in_every_element(ldpc, gpu, per):
    """parity_check_matrix(1000, 10, 9), 100 iterations (test/test_bf_decoder.jl), 2,048 columns, three tie rules, two seeds."""
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    B = 2048
    model = BitFlipModel(H, 100)
    stops_seen = set()
    for seed in (7, 2024):
        e, syn = _syndromes(ldpc, H, B, per, seed=seed + 1)
        for rule, tie in RULES.items():
            dec = ldpc.BitFlipDecoder(H, per, 100, tie_break=rule, seed=seed)
            assert dec.kernel == 1 and (dec.s, dec.n) == (900, 1000)
            got = dec.decode_batch_host(syn, column0=0)
            want = model.decode_batch(syn, tie, seed=seed)
            print(f"per {per} seed {seed} {rule}: recovered {int((got[0] == e).all(axis=1).sum())}/{B}, "
                  f"stop reasons {np.bincount(got[3], minlength=3).tolist()}, iterations {int(got[2].sum())}")
            _assert_equal_to_model(got, want, f"per {per} seed {seed} {rule}")
            stops_seen |= set(np.unique(got[3]).tolist())
            # converged is the reference's flag: 1 for reasons 1 and 2
            assert np.array_equal(got[1] != 0, got[3] != 0)
            if per == 0.01:
                # the reference's own bar (test/test_bf_decoder.jl:35): logical error rate < 0.005 at per 0.01
                assert (got[0] != e).any(axis=1).mean() < 0.005
            dec.close()
    assert 1 in stops_seen
    if per == 0.03:
        assert 0 in stops_seen, "no column ran out of iterations: the input exercises one stop reason only"


def test_tiers_agree_with_the_model_on_one_small_graph(ldpc, gpu):
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    B = 300
    _, syn = _syndromes(ldpc, H, B, 0.03, seed=5)
    want = BitFlipModel(H, 60).decode_batch(syn, TIE_RANDOM, seed=99)
    for variant in (1, 2, 3):
        dec = ldpc.BitFlipDecoder(H, 0.03, 60, seed=99, kernel_variant=variant)
        assert dec.kernel == variant
        _assert_equal_to_model(dec.decode_batch_host(syn, column0=0), want, f"tier {variant}")
        dec.close()


def test_workgroup_tier_on_a_graph_that_needs_it(ldpc, gpu):
    """(16384, 8, 4): 9 n + s bytes of state do not fit a wave's share of the LDS; one 16-wave workgroup per syndrome."""
    H = ldpc.codes.parity_check_csc(16384, 8, 4)
    B = 256
    _, syn = _syndromes(ldpc, H, B, 0.002, seed=21)
    for rule, tie in (("random", TIE_RANDOM), ("last", TIE_LAST)):
        dec = ldpc.BitFlipDecoder(H, 0.002, 80, tie_break=rule, seed=3)
        assert dec.kernel == 2
        got = dec.decode_batch_host(syn, column0=0)
        _assert_equal_to_model(got, BitFlipModel(H, 80).decode_batch(syn, tie, seed=3), f"(16384, 8, 4) {rule}")
        assert len(set(np.unique(got[3]).tolist())) >= 2   # more than one way to stop occurs
        dec.close()


@pytest.mark.parametrize("variant", [0, 2, 3])
def test_irregular_graph_with_a_degree_0_bit_and_a_degree_1_check(ldpc, gpu, variant):
    H = _irregular(1003, 518, 5)
    B = 256
    _, syn = _syndromes(ldpc, H, B, 0.01, seed=8)
    syn[3, 517] ^= 1    # the degree-1 check mismatched where its only bit is clean
    dec = ldpc.BitFlipDecoder(H, 0.01, 50, seed=1, kernel_variant=variant)
    assert dec.kernel == (variant or 1)
    _assert_equal_to_model(dec.decode_batch_host(syn, column0=0), BitFlipModel(H, 50).decode_batch(syn, TIE_RANDOM, seed=1), "irregular")
    dec.close()


def test_unlimited_tier_with_64_bit_votes(ldpc, gpu):
    """max_iters * max bit degree >= 2^31: create takes the 64-bit accumulators instead of wrapping."""
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    _, syn = _syndromes(ldpc, H, 80, 0.01, seed=4)
    # only columns that the model matches within 100 iterations (the trajectory does not depend on max_iters): with
    # 2^31 - 1 iterations a column that never matches would not end in the life of this test
    syn = syn[BitFlipModel(H, 100).decode_batch(syn, TIE_FIRST)[3] == 1]
    assert syn.shape[0] >= 64
    big = 2 ** 31 - 1
    dec = ldpc.BitFlipDecoder(H, 0.01, big, tie_break="first")
    assert dec.kernel == 4
    got = dec.decode_batch_host(syn, column0=0)
    _assert_equal_to_model(got, BitFlipModel(H, big).decode_batch(syn, TIE_FIRST), "64-bit votes")
    dec.close()


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_column0_makes_calls_independent_of_chunking_and_entry(ldpc, gpu, variant):
    import torch

    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    B = 130
    _, syn = _syndromes(ldpc, H, B, 0.03, seed=6)
    dec = ldpc.BitFlipDecoder(H, 0.03, 50, seed=42, kernel_variant=variant)
    want = BitFlipModel(H, 50).decode_batch(syn, TIE_RANDOM, seed=42, column0=1000)
    whole = dec.decode_batch_host(syn, column0=1000)
    _assert_equal_to_model(whole, want, "one call")
    _assert_equal_to_model(dec.decode_batch_host(syn, column0=1000), want, "the handle used twice")
    halves = [dec.decode_batch_host(syn[a:b], column0=1000 + a) for a, b in ((0, B // 2), (B // 2, B))]
    _assert_equal_to_model([np.concatenate(x) for x in zip(*halves)], want, "two halves")
    singles = [dec.decode_batch_host(syn[i:i + 1], column0=1000 + i) for i in range(B)]
    _assert_equal_to_model([np.concatenate(x) for x in zip(*singles)], want, "B calls of batch 1")
    # device entry, on a stream of its own and then on the default stream
    d_syn = torch.from_numpy(syn).cuda()
    for stream in (torch.cuda.Stream(), None):
        err = torch.full((B, dec.n), 9, dtype=torch.uint8, device="cuda")
        conv = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        stop = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        its = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if stream is None:
            dec.decode_batch_device(d_syn, err, conv, its, stop, column0=1000)
        else:
            with torch.cuda.stream(stream):
                dec.decode_batch_device(d_syn, err, conv, its, stop, column0=1000)
        torch.cuda.synchronize()
        _assert_equal_to_model((err.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy(), stop.cpu().numpy()), want, "device entry")
    # without the optional outputs
    err = torch.zeros((B, dec.n), dtype=torch.uint8, device="cuda")
    conv = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    dec.decode_batch_device(d_syn, err, conv, column0=1000)
    torch.cuda.synchronize()
    assert np.array_equal(err.cpu().numpy(), want[0]) and np.array_equal(conv.cpu().numpy(), want[1])
    dec.close()


@pytest.mark.parametrize("B", [1, 63, 65, 1027])
def test_ragged_batches(ldpc, gpu, B):
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    _, syn = _syndromes(ldpc, H, B, 0.02, seed=B)
    dec = ldpc.BitFlipDecoder(H, 0.02, 40, seed=B)
    got = dec.decode_batch_host(syn, column0=0)
    _assert_equal_to_model(got, BitFlipModel(H, 40).decode_batch(syn, TIE_RANDOM, seed=B), f"batch {B}")
    dec.close()


def test_every_candidate_is_taken_under_random_and_first_last_agree(ldpc, gpu):
    """The same syndrome in every column; iteration 1 has k >= 2 candidates (the model tells k).  Under RANDOM the first
    flip of column i is candidate random_rank(seed, i, 1, k); with B columns the chance that some candidate is never
    drawn is at most k (1 - 1/k)^B, and B is sized so that this is below 1e-9."""
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    e = np.zeros((1, 1000), dtype=np.uint8)
    e[0, [17, 400]] = 1
    syn1 = ldpc.codes.syndromes_of(H, e)[0]
    model = BitFlipModel(H, 1)
    trace = []
    model.decode(syn1, chooser_for(TIE_FIRST), trace=trace)
    cand = trace[0][2]
    k = len(cand)
    assert k >= 2
    B = 1
    while k * (1 - 1 / k) ** B >= 1e-9:
        B += 1
    print(f"k = {k} candidates {cand.tolist()}, B = {B}")
    syn = np.tile(syn1, (B, 1))
    dec = ldpc.BitFlipDecoder(H, 0.01, 1, seed=77)   # one iteration: the output is the first flip
    err, conv, its, stop = dec.decode_batch_host(syn, column0=0)
    assert (err.sum(axis=1) == 1).all() and (its == 1).all() and (stop == 0).all() and not conv.any()
    first = err.argmax(axis=1)
    assert np.array_equal(first, [cand[random_rank(77, i, 1, k)] for i in range(B)])
    assert set(first.tolist()) == set(cand.tolist())
    dec.close()
    for rule, want in (("first", cand[0]), ("last", cand[-1])):
        dec = ldpc.BitFlipDecoder(H, 0.01, 1, tie_break=rule, seed=77)
        err = dec.decode_batch_host(syn[:200], column0=0)[0]
        assert (err.sum(axis=1) == 1).all() and (err.argmax(axis=1) == want).all()
        dec.close()


def test_edge_inputs(ldpc, gpu):
    H = ldpc.codes.parity_check_csc(1000, 10, 9)
    _, syn = _syndromes(ldpc, H, 40, 0.01, seed=2)
    syn[0, 3] = 2
    syn[1, 899] = 3
    syn[2, :] = 0
    syn[3, :] = 2
    for variant in (1, 2, 3):
        dec = ldpc.BitFlipDecoder(H, 0.01, 30, seed=9, kernel_variant=variant)
        got = dec.decode_batch_host(syn, column0=0)
        _assert_equal_to_model(got, BitFlipModel(H, 30).decode_batch(syn, TIE_RANDOM, seed=9), "entries 2 and 3")
        assert got[3][0] == 0 and got[2][0] == 30 and got[1][0] == 0       # never matches: runs to max_iters
        assert got[3][1] == 0 and got[2][1] == 30
        assert got[3][2] == 1 and got[2][2] == 1 and not got[0][2].any()   # all-zero syndrome: 1 iteration, zeros
        assert dec.decode_batch_host(syn[:0], column0=0)[0].shape == (0, 1000)   # batch 0
        dec.close()
    for max_iters in (0, 1):
        dec = ldpc.BitFlipDecoder(H, 0.01, max_iters, seed=9)
        got = dec.decode_batch_host(syn, column0=0)
        _assert_equal_to_model(got, BitFlipModel(H, max_iters).decode_batch(syn, TIE_RANDOM, seed=9), f"max_iters {max_iters}")
        if max_iters == 0:
            assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
        dec.close()
    # stop reason 2 on the 3 x 3 all-ones graph: every vote is +1 - 1 - 1 = -1; the reference then reports converged
    H3 = np.ones((3, 3), dtype=np.bool_)
    syn3 = np.array([[1, 0, 0], [1, 1, 1], [0, 0, 0], [2, 1, 1]], dtype=np.uint8)
    for variant in (1, 2, 3):
        dec = ldpc.BitFlipDecoder(H3, 0.01, 10, tie_break="first", kernel_variant=variant)
        got = dec.decode_batch_host(syn3, column0=0)
        _assert_equal_to_model(got, BitFlipModel(H3, 10).decode_batch(syn3, TIE_FIRST), "3 x 3")
        assert got[3].tolist() == [2, 1, 1, 0] and got[1].tolist() == [1, 1, 1, 0] and got[2].tolist() == [1, 2, 1, 10]
        assert got[0].tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]]
        dec.close()
    # s = 0: nothing to match, converged at once; n = 0: no bit at all (reason 1 for a zero syndrome, 2 otherwise)
    dec = ldpc.BitFlipDecoder(sp.csc_matrix((0, 5), dtype=np.uint8), 0.01, 4)
    err, conv, its, stop = dec.decode_batch_host(np.zeros((3, 0), dtype=np.uint8), column0=0)
    assert err.shape == (3, 5) and not err.any() and conv.all() and (its == 1).all() and (stop == 1).all()
    dec.close()
    dec = ldpc.BitFlipDecoder(sp.csc_matrix((4, 0), dtype=np.uint8), 0.01, 4)
    syn0 = np.array([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=np.uint8)
    got = dec.decode_batch_host(syn0, column0=0)
    _assert_equal_to_model(got, BitFlipModel(sp.csc_matrix((4, 0), dtype=np.uint8), 4).decode_batch(syn0), "n = 0")
    assert got[3].tolist() == [1, 2]
    dec.close()


def test_python_mirror(ldpc, gpu):
    H = ldpc.parity_check_matrix(1000, 10, 9)
    Hs = ldpc.codes.parity_check_csc(1000, 10, 9)
    e, syn = _syndromes(ldpc, Hs, 12, 0.01, seed=31)
    model = BitFlipModel(Hs, 100)
    dec = ldpc.BitFlipDecoder(H, 0.01, 100, seed=5)
    assert (dec.per, dec.max_iters, dec.s, dec.n) == (0.01, 100, 900, 1000) and dec.sparse_H.shape == (900, 1000)
    assert dec.scratch.err.shape == (1000,) and dec.scratch.votes.shape == (1000,) and dec.columns_decoded == 0
    # decode_ numbers its columns: the same syndrome twice is column 0, then column 1
    for c in range(2):
        guess, ok = dec.decode_(syn[0])
        werr, wconv, _, _ = model.decode(syn[0], chooser_for(TIE_RANDOM, 5), column=c)
        assert guess.dtype == np.int64 and np.array_equal(guess, werr) and ok is bool(wconv) and guess is dec.scratch.err
        assert dec.columns_decoded == c + 1
    with pytest.raises(IndexError):
        dec.decode_(syn[0][:-1])
    # batchdecode_: s x B in, n x B out, columns 2 .. 13
    errors = np.zeros((1000, 12), dtype=np.bool_)
    out, success = ldpc.batchdecode_(dec, syn.T.astype(np.bool_), errors)
    want = model.decode_batch(syn, TIE_RANDOM, seed=5, column0=2)
    assert out is errors and success.dtype == np.bool_ and dec.columns_decoded == 14
    assert np.array_equal(errors.T.astype(np.uint8), want[0]) and np.array_equal(success, want[1].astype(bool))
    # a fixed seed replays a session
    dec2 = ldpc.BitFlipDecoder(H, 0.01, 100, seed=5)
    dec2.columns_decoded = 2
    again = np.zeros((1000, 12), dtype=np.int64)
    dec2.batchdecode_(syn.T, again, np.zeros(12, dtype=np.bool_))
    assert np.array_equal(again, errors.astype(np.int64))
    # the reference's two assertions (:190-191)
    with pytest.raises(AssertionError):
        dec.batchdecode_(syn.T, np.zeros((1000, 11), dtype=np.uint8))
    with pytest.raises(AssertionError):
        dec.batchdecode_(syn.T, np.zeros((1000, 12), dtype=np.uint8), np.zeros(11, dtype=np.bool_))
    # stored zeros of a sparse H are not edges
    Hz = sp.csc_matrix(Hs, copy=True).astype(np.uint8)
    Hz.data[::7] = 0
    dz = ldpc.BitFlipDecoder(Hz, 0.01, 20, tie_break="last")
    Hd = sp.csc_matrix(Hz, copy=True); Hd.eliminate_zeros()
    assert dz.sparse_H.nnz == Hd.nnz < Hs.nnz
    _assert_equal_to_model(dz.decode_batch_host(syn, column0=0), BitFlipModel(Hd, 20).decode_batch(syn, TIE_LAST), "stored zeros")
    dz.close(); dec.close(); dec2.close()


def test_c_host_decodes_on_the_gpu(ldpc, gpu, tmp_path):
    """tests/abi_bitflip_driver.c "gpu": hand-checked cases of the 3 x 3 graph, and the RANDOM rule against ranks the
    model computes here (column0 = 5, three candidates in iteration 1)."""
    from test_bitflip_cpu import _build_driver

    exe = _build_driver(tmp_path)
    seed, B = 123456789, 24
    want = [str(random_rank(seed, 5 + i, 1, 3)) for i in range(B)]
    assert len(set(want)) == 3
    out = subprocess.run([exe, "gpu", str(seed), str(B)] + want, capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
