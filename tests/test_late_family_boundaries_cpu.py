"""The preconditions of tests/test_gpu_late_family_boundaries.py without a GPU: every assertion that a case makes on the
priors or on its numpy model before it touches the device, so that a fixture that stops reaching its path fails on any
machine.  Neither the library nor torch is touched."""
import pytest

import test_gpu_late_family_boundaries as late


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_the_decimation_cases_reach_their_paths(case):
    late.decim_preconditions(case)


@pytest.mark.parametrize("alpha,clamped", [(0.75, False), (1.0, False), (1.0, True)])
def test_the_pauli_relay_cases_reach_their_paths(alpha, clamped):
    late.pauli_relay_preconditions(alpha, clamped)


def test_the_relay_case_reaches_its_paths():
    late.relay_preconditions()
