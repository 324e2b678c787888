"""The one step of the BP decode (ldpc_mi355x.hip, decode_device_impl) that no other test executes: dump_team_debug(), the
LDPC_TEAM_DEBUG diagnostics after a team grid's fresh pass.  (The refused-team-grid fallback cannot be reached without
making the runtime fail and stays untested.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_team_debug_dump_runs_and_changes_nothing(ldpc, gpu, monkeypatch, capfd):
    """(3,6) n = 1008, 257 syndromes (four tiles and one), the experiments build's knobs as test_gpu_team_matrix.py sets
    them (teams of four on a small graph, rows in LDS and registers) and LDPC_TEAM_DEBUG=1: the call waits for the stream,
    reads every team's control block back and prints where the teams ran.  The dump must have run (its first line names
    the launch: 5 tiles, 8 teams x 4 workgroups) and the results must be, bit for bit, those of the tile kernel without
    hand-off (kernel_variant=1, defer_threshold=-1) -- hard decisions, flags, iteration counts, LLR bits."""
    n, B, per, iters = 1008, 257, 0.04, 30
    H = ldpc.codes.parity_check_csc(n, 6, 3)
    syn = ldpc.codes.syndromes_of(H, ldpc.codes.random_errors(n, B, per, seed=257))
    for k, v in (("LDPC_TEAM_MIN_ROWS", "1"), ("LDPC_TEAM_MAX", "4"), ("LDPC_TEAM_REGS", "32")):
        monkeypatch.setenv(k, v)
    ref_dec = ldpc.BeliefPropagationDecoder(H, per, iters, kernel_variant=1, defer_threshold=-1)
    ref = ref_dec.decode_batch_host(syn, want_llr=True, want_iters=True)
    assert ref_dec.info().last_kernel == 1
    ref_dec.close()
    assert 0 < ref[1].sum() and len(np.unique(ref[3])) > 3      # tiles of different iteration counts

    monkeypatch.setenv("LDPC_TEAM_DEBUG", "1")                   # read per call
    capfd.readouterr()
    dec = ldpc.BeliefPropagationDecoder(H, per, iters, kernel_variant=4)
    got = dec.decode_batch_host(syn, want_llr=True, want_iters=True)
    info = dec.info()
    dec.close()
    printed = capfd.readouterr().err
    assert info.last_kernel == 4 and info.last_team_size == 4 and info.last_lds_rows > 0, \
        (info.last_kernel, info.last_team_size, info.last_lds_rows)
    assert "[ldpc] team kernel: 5 tiles, 8 teams x 4 workgroups, grid 32;" in printed, printed
    assert sum(line.startswith("[ldpc]   team ") for line in printed.splitlines()) == 5, printed   # one line per team with a tile
    for a, b, name in zip(got, ref, ("hard decisions", "converged", "LLR bits", "iterations")):
        a, b = (a.view(np.int64), b.view(np.int64)) if name == "LLR bits" else (a, b)
        assert np.array_equal(a, b), f"{name} differ between the team kernel under LDPC_TEAM_DEBUG and the tile kernel"
