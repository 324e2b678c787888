"""BP-OTS on the MI355X at EVERY tile width, LDS budget, degree bucket, launch path and kernel boundary, against the CPU
oracle (oracle/bpots_oracle.c): equality in every element of errors, flags and iteration counts -- kernel and oracle share
portable_math.h, so there is no tolerance.  Never against another GPU run.

Before the GPU is touched every case asserts, through ldpc_debug_bpots_plan, the path it is there for; afterwards it
asserts through `dec.kernel` and ldpc_debug_bpots_last_launch that the handle took it.  So a case that misses its width,
its bucket or its launch path fails instead of passing on another one.

  a. tile widths: the rows of tests/test_bpots_plan_cpu.py's table with S = 64 ... 2, S = 1 inside 76 KiB (n = 504 and the
     last such n, 606) and inside 156 KiB (the first such n, 612, and 1200); batches 1, S - 1, S + 1, 2 S + 1 through the
     host entry (latency path) and the device entry on a side stream with poisoned outputs (queue path);
  b. more groups than workgroups (chunk 1), and groups taken from the queue in chunks (chunk >= 2);
  c. the four instantiations <8|32, 4|16> of the LDS and of the node kernel, and the steps 8 -> 9, 4 -> 5, 32 -> 33,
     16 -> 17, on a graph with one heavy check and one heavy bit whose last edge provably matters;
  d. LDS -> node and node -> unlimited by size, at the last and the first n of each;
  e. T = 1, T > max_iters, C = 0, per = 1e-6, 0.75 (prior exactly 0), 0.9 and 1 (negative prior); a graph without edges.

Inputs and oracle results come from tests/bpots_cases.py (pools of at most 48 distinct syndromes; a large batch repeats
them).  Oracle time per test: well under a second, except the two n ~ 23,600 graphs (about 1 s each)."""
import numpy as np
import pytest

import bpots_cases as bc

pytestmark = pytest.mark.gpu

LAT, QUEUE = 1, 2


def same(got, pool, idx, what):
    err, conv, its = got
    assert err.shape == (len(idx), pool.H.shape[1]) and conv.shape == its.shape == (len(idx),)
    bad = np.nonzero((err != pool.err[idx]).any(axis=1) | (conv != pool.conv[idx]) | (its != pool.its[idx]))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(idx)} columns differ from the oracle, first {bad[:6].tolist()}"


def host_entry(dec, pool, idx, what, path):
    got = dec.decode_batch_host(pool.syn[idx])
    same(got, pool, idx, what + " host")
    assert dec.last_launch().path == path, (what, dec.last_launch())
    return dec.last_launch()


def device_entry(dec, pool, idx, what, want_iters=True):
    """The device entry on a side stream, every output pre-filled with a value no decode writes."""
    import torch

    B = len(idx)
    side = torch.cuda.Stream()
    d_syn = torch.from_numpy(np.ascontiguousarray(pool.syn[idx])).cuda()
    err = torch.full((B, dec.n), 7, dtype=torch.uint8, device="cuda")
    conv = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_iters else None
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dec.decode_batch_device(d_syn, err, conv, its, stream=side.cuda_stream)
    side.synchronize()
    e, c = err.cpu().numpy(), conv.cpu().numpy()
    i = its.cpu().numpy() if want_iters else pool.its[idx]      # iters = NULL: nothing to compare
    same((e, c, i), pool, idx, what + " device")
    launch = dec.last_launch()
    assert launch.path == QUEUE, (what, launch)
    return launch


def assert_pool_is_mixed(pool):
    """On the oracle alone: converged and unconverged syndromes, one with entries 0 / 1 only that ran past T unconverged (a
    bias step), and syndromes with an entry of 2 and of 3 (which batches hold them is asserted per batch)."""
    assert 0 < int(pool.conv.sum()) < len(pool.conv)
    assert ((pool.its > pool.T) & (pool.conv == 0) & ~pool.wild).any()
    assert (pool.syn == 2).any() and (pool.syn == 3).any() and not pool.conv[pool.wild].any()


# ---- a. every tile width ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(bc.WIDTHS))
def test_every_tile_width_and_budget_equals_the_oracle(ldpc, gpu, n):
    S, budget = bc.WIDTHS[n][:2]
    pool = bc.width_pool(n)
    assert_pool_is_mixed(pool)
    plan = ldpc.bpots.bpots_plan_of(pool.H)
    assert (plan.kernel, plan.S, plan.budget_kib, plan.DC, plan.DV) == (2, S, budget, 8, 4)
    dec = pool.decoder(ldpc)
    assert dec.kernel == 2 and dec.last_launch().path == 0
    batches = [B for B in (1, S - 1, S + 1, 2 * S + 1) if B > 0]
    for k, B in enumerate(batches):
        idx = pool.batch(B)
        assert (pool.syn[idx] > 1).any()                        # every batch, through both routes, decodes an entry above 1
        if B >= 2:
            assert 0 < int(pool.conv[idx].sum()) < B            # mixed inside the batch
        if B >= 3:
            assert (pool.syn[idx] == 2).any() and (pool.syn[idx] == 3).any()
        groups = -(-B // S)
        launch = host_entry(dec, pool, idx, f"n={n} B={B}", LAT)
        assert (launch.groups, launch.grid, launch.chunk) == (groups, groups, 1)
        launch = device_entry(dec, pool, idx, f"n={n} B={B}", want_iters=(k != len(batches) - 1))
        assert (launch.groups, launch.grid, launch.chunk) == (groups, groups, 1) and launch.per_cu >= 1
        if 2 * plan.lds_bytes > 160 * 1024:                     # a CU has 160 KiB of LDS: such a request leaves room for one
            assert launch.per_cu == 1                           # (n = 1200; at n = 612 two requests of 70 KiB still fit)
    if n == 1200:   # a host batch whose image is past 256 KiB leaves the latency path
        idx = pool.batch(150, seed=3)
        assert 150 * (pool.H.shape[0] + n + 5) > 256 * 1024 and (pool.syn[idx] > 1).any()
        launch = host_entry(dec, pool, idx, "n=1200 B=150", QUEUE)
        assert (launch.groups, launch.grid, launch.chunk) == (150, 150, 1)
    # host, device and host again on the one handle
    idx = pool.batch(2 * S + 1, seed=n)
    assert (pool.syn[idx] == 2).any() and (pool.syn[idx] == 3).any()
    host_entry(dec, pool, idx, f"n={n} again", LAT)
    device_entry(dec, pool, idx, f"n={n} again")
    host_entry(dec, pool, idx, f"n={n} again", LAT)
    dec.close()


# ---- b. more groups than workgroups, and chunks -----------------------------------------------------------------------

def test_more_groups_than_workgroups_and_chunked_queue(ldpc, gpu):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # chunk 1: workgroups come back to the queue for further groups
    pool = bc.width_pool(504, 3, 2)
    assert 0 < int(pool.conv.sum()) < len(pool.conv) and (pool.its > pool.T).any()
    assert ldpc.bpots.bpots_plan_of(pool.H)[:2] == (2, 1)
    dec = pool.decoder(ldpc)
    per_cu = device_entry(dec, pool, pool.batch(3), "n=504 first").per_cu
    assert per_cu >= 1
    B = per_cu * cus + 90
    launch = device_entry(dec, pool, pool.batch(B, seed=1), f"n=504 B={B}")
    assert launch.groups == B and launch.grid == per_cu * cus and launch.groups > launch.grid and launch.chunk == 1
    dec.close()
    # chunk >= 2: 32 groups a workgroup
    pool = bc.width_pool(1200, 3, 2)
    assert 0 < int(pool.conv.sum()) < len(pool.conv) and (pool.its > pool.T).any()
    plan = ldpc.bpots.bpots_plan_of(pool.H)
    assert (plan.kernel, plan.S, plan.budget_kib) == (2, 1, 156)
    dec = pool.decoder(ldpc)
    per_cu = device_entry(dec, pool, pool.batch(3), "n=1200 first").per_cu
    assert per_cu == 1
    B = 32 * per_cu * cus + 3
    launch = device_entry(dec, pool, pool.batch(B, seed=2), f"n=1200 B={B}")
    assert launch.groups == B and launch.grid == per_cu * cus and launch.chunk >= 2
    dec.close()


# ---- c. degree buckets --------------------------------------------------------------------------------------------------

def _last_edge_matters(pool, chk, bit):
    """On the CPU: the oracle on the same graph without the heavy check's last edge, and without the heavy bit's, answers
    differently for some syndrome of the batch -- a kernel that dropped either edge could not equal the oracle."""
    H = np.asarray(pool.H.todense())
    for kw in ({"chk": chk}, {"bit": bit}):
        o = bc.oracle_decode(bc.without_last_edge(H, **kw), pool.per, pool.iters, pool.T, pool.C, pool.syn)
        assert ((o[0] != pool.err).any(axis=1) | (o[1] != pool.conv) | (o[2] != pool.its)).any(), kw


@pytest.mark.parametrize("d,e", bc.BUCKET_PAIRS)
def test_every_degree_bucket_of_the_lds_and_the_node_kernel(ldpc, gpu, monkeypatch, d, e):
    pool, chk, bit = bc.bucket_pool(120, d, e)
    assert 0 < int(pool.conv.sum()) < len(pool.conv) and ((pool.its > pool.T) & (pool.conv == 0)).any()
    _last_edge_matters(pool, chk, bit)
    DC, DV = bc.bucket_of(d, e)
    idx = pool.batch(len(pool.syn))
    plan = ldpc.bpots.bpots_plan_of(pool.H)
    assert (plan.kernel, plan.DC, plan.DV) == (2, DC, DV) and plan.S in (4, 8)
    dec = pool.decoder(ldpc)
    assert dec.kernel == 2
    host_entry(dec, pool, idx, f"lds <{DC},{DV}>", LAT)
    device_entry(dec, pool, idx, f"lds <{DC},{DV}>")
    dec.close()
    for force, kernel, buckets in ((1, 3, (DC, DV)), (2, 5, (0, 0))):
        plan = ldpc.bpots.bpots_plan_of(pool.H, force_node=force)
        assert (plan.kernel, plan.DC, plan.DV) == (kernel,) + buckets
        monkeypatch.setenv("LDPC_BPOTS_FORCE_NODE", str(force))
        dec = pool.decoder(ldpc)
        monkeypatch.delenv("LDPC_BPOTS_FORCE_NODE")
        assert dec.kernel == kernel
        launch = host_entry(dec, pool, idx, f"kernel {kernel} <{DC},{DV}>", QUEUE)
        assert (launch.groups, launch.grid, launch.chunk, launch.per_cu) == (len(idx), len(idx), 1, 0)
        device_entry(dec, pool, idx, f"kernel {kernel} <{DC},{DV}>", want_iters=False)
        dec.close()


@pytest.mark.parametrize("d,e", bc.WIDE_PAIRS)
def test_one_edge_past_the_buckets_takes_the_unlimited_kernel(ldpc, gpu, d, e):
    pool, chk, bit = bc.bucket_pool(120, d, e)
    assert 0 < int(pool.conv.sum()) < len(pool.conv) and ((pool.its > pool.T) & (pool.conv == 0)).any()
    _last_edge_matters(pool, chk, bit)
    for force in (0, 1, 2):
        assert ldpc.bpots.bpots_plan_of(pool.H, force_node=force) == (5, 0, 0, 0, 0, 0)
    idx = pool.batch(len(pool.syn))
    dec = pool.decoder(ldpc)
    assert dec.kernel == 5
    host_entry(dec, pool, idx, f"wide {d},{e}", QUEUE)
    device_entry(dec, pool, idx, f"wide {d},{e}")
    dec.close()


# ---- d. kernel boundaries by size ---------------------------------------------------------------------------------------

def _by_size(ldpc, pool, kernel, lds_budget=None):
    plan = ldpc.bpots.bpots_plan_of(pool.H)
    assert plan.kernel == kernel and (plan.DC, plan.DV) == ((8, 4) if kernel != 5 else (0, 0))
    assert ((pool.its > pool.T) & (pool.conv == 0)).any() and 0 < int(pool.conv.sum()) < len(pool.conv)
    idx = pool.batch(len(pool.syn))
    dec = pool.decoder(ldpc)
    assert dec.kernel == kernel
    device_entry(dec, pool, idx, f"n={pool.H.shape[1]} kernel {kernel}")
    host_entry(dec, pool, idx, f"n={pool.H.shape[1]} kernel {kernel}", LAT if kernel == 2 and len(idx) * (pool.H.shape[0] + pool.H.shape[1] + 5) <= 250 * 1024 else QUEUE)
    dec.close()
    return plan


def test_lds_to_node_kernel_at_the_last_and_the_first_size(ldpc, gpu):
    plan = _by_size(ldpc, bc.regular_pool(1500, 24, 0.06, 8, 3), 2)
    assert (plan.S, plan.budget_kib, plan.lds_bytes + 8192) == (1, 156, 159128)
    plan = _by_size(ldpc, bc.regular_pool(1512, 24, 0.06, 8, 3), 3)
    assert plan.lds_bytes == ((756 + 3 * 1512 + 15) // 16) * 16 + 4 * 756 + 28 * 1024 + 64


def test_node_to_unlimited_kernel_at_the_last_and_the_first_size(ldpc, gpu):
    n = 23400
    while ldpc.bpots.bpots_plan(n // 2 + 3, n + 6, 3 * n + 18, 6, 3).kernel == 3:
        n += 6
    assert 23400 < n < 23800 and ldpc.bpots.bpots_plan(n // 2, n, 3 * n, 6, 3).kernel == 3
    _by_size(ldpc, bc.regular_pool(n, 6, 0.05, 6, 2), 3)
    _by_size(ldpc, bc.regular_pool(n + 6, 6, 0.05, 6, 2), 5)


def test_node_kernel_of_natural_size_with_heavy_nodes(ldpc, gpu):
    """n = 1800 is beyond the LDS kernel; one check of 32 and one bit of 16 edges: bpots_node_kernel<32, 16>, not forced."""
    H, chk, bit = bc.widened(1800, 32, 16)
    E = ldpc.codes.random_errors(1800, 24, 0.055, seed=18)
    E[:8] &= ldpc.codes.random_errors(1800, 8, 0.6, seed=19)
    E[:, bit] |= (np.arange(24) % 3 == 0).astype(np.uint8)
    pool = bc.Pool(H, 0.055, 8, 2, 2.0, ldpc.codes.syndromes_of(H, E))
    assert 0 < int(pool.conv.sum()) < 24 and ((pool.its > pool.T) & (pool.conv == 0)).any()
    _last_edge_matters(pool, chk, bit)
    plan = ldpc.bpots.bpots_plan_of(pool.H)
    assert (plan.kernel, plan.DC, plan.DV) == (3, 32, 16)
    dec = pool.decoder(ldpc)
    assert dec.kernel == 3
    idx = pool.batch(24)
    device_entry(dec, pool, idx, "n=1800 <32,16>")
    host_entry(dec, pool, idx, "n=1800 <32,16>", QUEUE)
    dec.close()


# ---- e. parameters ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["irregular", "bb72"])
def test_parameter_edges_equal_the_oracle(ldpc, gpu, name):
    """per in {1e-6, 0.75, 0.9, 1} x T in {1, max_iters + 5} x C in {0, 2}; tests/test_bpots_oracle.py holds the oracle
    against its second witness on the same inputs."""
    seen = set()
    for per, T, C in bc.param_cases():
        pool = bc.param_pool(name, per, T, C)
        plan = ldpc.bpots.bpots_plan_of(pool.H)
        assert plan.kernel == 2 and plan.S >= 16
        idx = pool.batch(len(pool.syn))
        dec = pool.decoder(ldpc)
        host_entry(dec, pool, idx, f"{name} per={per} T={T} C={C}", LAT)
        device_entry(dec, pool, idx, f"{name} per={per} T={T} C={C}")
        dec.close()
        seen.add((int(pool.conv.sum()), int(pool.err.sum()), tuple(sorted(set(pool.its.tolist())))))
        if per == 0.75:     # the prior is exactly 0: with no syndrome bit set every LLR is 0 and no decision is 1
            assert not pool.err[0].any() and pool.conv[0] == 1 and pool.its[0] == 1
    assert len(seen) >= 4       # the parameters change what the oracle answers


def test_a_graph_without_edges(ldpc, gpu):
    H = np.zeros((3, 5), dtype=np.uint8)
    syn = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 2, 0], [1, 1, 1], [0, 0, 0], [0, 0, 3]], dtype=np.uint8)
    pool = bc.Pool(H, 0.05, 7, 2, 2.0, syn)
    zero = ~syn.any(axis=1)
    assert np.array_equal(pool.conv, zero.astype(np.uint8)) and np.array_equal(pool.its, np.where(zero, 1, 7)) and not pool.err.any()
    assert ldpc.bpots.bpots_plan_of(H)[:2] == (2, 64)
    idx = np.arange(len(syn))
    dec = pool.decoder(ldpc)
    assert dec.kernel == 2
    host_entry(dec, pool, idx, "no edges", LAT)
    device_entry(dec, pool, idx, "no edges")
    got = dec.decode_batch_host(syn)
    assert not got[0].any() and np.array_equal(got[1], zero.astype(np.uint8)) and np.array_equal(got[2], np.where(zero, 1, 7))
    dec.close()
