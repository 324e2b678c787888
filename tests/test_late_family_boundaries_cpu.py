"""The preconditions of tests/test_gpu_late_family_boundaries.py without a GPU: every assertion that a case makes on the
priors or on its numpy model before it touches the device, so that a fixture that stops reaching its path fails on any
machine.  Neither the library nor torch is touched.

The last two tests pin what the relay cases of that file reach without saying so: lanes that find a solution in the MIDDLE of
a leg and go on -- the `restart` path of relay_kernels.hpp, after which the first sweep of the next leg reads every record
form (checks of degree 31 ... 65 on these graphs) as zeros (`fresh`) one round later than at a leg's natural end."""
import numpy as np
import pytest

import test_gpu_late_family_boundaries as late
from pauli_model import pauli_priors
from pauli_relay_model import PauliRelayModel
from relay_model import RelayModel
from test_gpu_family_boundaries import family_edges, pauli_edges


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_the_decimation_cases_reach_their_paths(case):
    late.decim_preconditions(case)


@pytest.mark.parametrize("alpha,clamped", [(0.75, False), (1.0, False), (1.0, True)])
def test_the_pauli_relay_cases_reach_their_paths(alpha, clamped):
    late.pauli_relay_preconditions(alpha, clamped)


def test_the_relay_case_reaches_its_paths():
    late.relay_preconditions()


def mid_leg_restarts(steps, iters, leg_iters):
    """steps: per iteration (leg [B], iterations done in the leg [B], hit [B]); iters [B]: the iterations a lane ran.
    -> per lane, the solutions found before the leg had used up its iterations after which the lane ran on."""
    out = np.zeros(len(iters), dtype=np.int64)
    for k, (leg, t, hit) in enumerate(steps):
        out += hit & (k + 1 < iters) & (t < np.asarray(leg_iters)[leg])
    return out


def test_the_relay_case_restarts_in_the_middle_of_a_leg():
    H, _, prior, syn = family_edges()[:4]
    g, want = late.relay_want()
    steps = []
    again = RelayModel(H, prior, g, late.RL_LEGS, stop_after=2).decode(np.array(syn), steps=steps)
    assert all(np.array_equal(x, y) for x, y in zip(again, want))
    n = mid_leg_restarts(steps, want[2], late.RL_LEGS)
    assert (n > 0).sum() == 13, n.tolist()


@pytest.mark.parametrize("alpha", [0.75, 1.0])
def test_the_pauli_relay_case_restarts_in_the_middle_of_a_leg(alpha):
    Hx, Hz, probs, sx, sz = pauli_edges()
    want = late.pauli_relay_want(alpha, False)
    trace = []
    again = PauliRelayModel(Hx, Hz, pauli_priors(probs), late.pauli_relay_gammas(), late.PR_LEGS, alpha=alpha, clip=1e6,
                            stop_after=late.PR_STOP).decode(sx, sz, trace=trace)
    assert all(np.array_equal(x, y) for x, y in zip(again, want))
    n = mid_leg_restarts(trace, want[3], late.PR_LEGS)
    assert (n > 0).any(), "no lane finds a solution in the middle of a leg and goes on"
