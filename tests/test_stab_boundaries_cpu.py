"""Every precondition of tests/test_gpu_stab_boundaries.py without a GPU: the fixtures' first-sweep values from the priors
and the edge types alone, the model's outputs, the exact tie tables and their letters.  Nothing here calls the library's
decoders; the GPU file runs the same functions before it touches the GPU."""
import numpy as np
import pytest

import test_gpu_stab_boundaries as sb
from pauli_model import pauli_priors
from stab_model import TX, TY, TZ, StabMinSumModel


def test_the_first_sweep_of_the_fixture_from_the_priors_alone():
    sb.stab_edges_reach_their_paths()
    Sx, Sz, probs, s = sb.stab_edges()
    assert s.shape == (sb.B, sb.R) == (65, 30) and Sx.shape == Sz.shape == (30, 300)
    A, Z = Sx.toarray().astype(bool), Sz.toarray().astype(bool)
    assert min((A & ~Z).sum(), (Z & ~A).sum(), (A & Z).sum()) > 100            # all three edge types, many of each
    assert ((A.astype(int) @ Z.T + Z.astype(int) @ A.T) % 2).any()             # the rows do not commute: check=False
    clip = sb.clamp_clip()
    assert abs(clip - 0.04) < 1e-6                                            # half of |-0.04 * 2|, the last qubit of check 2


def test_stab_first_sweep_equals_the_first_check_sweep_of_the_model():
    """stab_first_sweep restates the header's rule for sweep 1; the model's messages after ONE iteration follow from its b:
    c_k = +-alpha * (k == a ? m2 : m1) with the sign par ^ neg_k."""
    Sx, Sz, probs, s = sb.stab_edges()
    priors = pauli_priors(probs)
    model = StabMinSumModel(Sx, Sz, priors, 1, alpha=0.75)
    model.decode(s)
    b = sb.stab_first_sweep(priors, model.rows, model.types, 1e6)
    for i in sb.WIDE:
        mag, neg = np.abs(b[i]), b[i] < 0
        order = np.argsort(mag, kind="stable")
        m1, m2, a = mag[order[0]], mag[order[1]], order[0]
        val = np.float32(0.75) * np.where(np.arange(len(mag)) == a, m2, m1)
        par = (s[:, i] != 0) ^ (neg.sum() % 2 == 1)
        want = np.where(par[:, None] ^ neg[None, :], -val[None, :], val[None, :]).astype(np.float32)
        assert np.array_equal(sb.bits(model.last_messages[i]), sb.bits(want)), i


@pytest.mark.parametrize("alpha, clamped", sb.CASES)
def test_the_record_form_cases_reach_their_paths_on_the_model(alpha, clamped):
    gx, gz, conv, its, G = sb.record_preconditions(alpha, clamped)
    print(f"alpha {alpha} clamped {clamped}: converged {int(conv.sum())} of {sb.B}, iteration counts {sorted(set(its.tolist()))}")


def test_the_tie_tables_and_their_letters():
    sb.ties_preconditions()
    Sx, Sz, probs, s, want, messages = sb.ties_case()
    assert Sx.shape == (4, 23) and s.shape == (16, 4) and len(sb.TIES) == len(sb.TIE_LETTERS) == 16 >= 13
    T = Sx.toarray() + 2 * Sz.toarray()
    assert not T[:, :16].any() and (T[:, 16:] != 0).sum(axis=0).min() >= 1     # 16 isolated qubits, 7 connected ones
    assert {TX, TY, TZ} == set(T[T != 0].tolist())
