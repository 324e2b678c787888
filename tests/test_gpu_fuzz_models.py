"""A short run of tools/fuzz_models.py: random Tanner graphs (irregular with empty and heavy nodes and sizes at the word
boundaries, small Gallager codes), ragged batches, every kernel_variant that create accepts, the bit-flip, min-sum, relay,
device OSD, trials and CSS trials kernels compared in every element with their numpy models, the three BP-OTS kernels
(tiers 2, 3, 5: LDS-resident, node-parallel, unlimited) with the C oracle, the guided-decimation min-sum kernels (tiers 1
and 2), the Pauli relay min-sum kernels (tiers 1 and 2), the OSD step by the standard rule (tiers 1, 2, 3) and the
stabilizer (non-CSS) min-sum kernels (tiers 1 and 2) with their numpy models.  (`relay tiers` is a substring of `pauli_relay tiers`: the patterns are anchored on the separator.)"""
import os
import re
import subprocess
import sys

import pytest

from test_fuzz_models_cpu import CASES, SEEDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = {"bitflip": {1, 2, 3}, "minsum": {1, 2}, "relay": {1, 2}, "osd": {1, 2, 3}, "trials": {1, 2}, "css": {1, 2},
         "layered": {1, 2}, "priors": {1, 2}, "pauli": {1, 2}, "bpots": {2, 3, 5}, "decim": {1, 2}, "pauli_relay": {1, 2},
         "osd_search": {1, 2, 3}, "stab": {1, 2}}
_REPORTS = {}


def _run(seed):
    if seed not in _REPORTS:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_models.py"), str(CASES), str(seed)],
                             capture_output=True, text=True, cwd=ROOT, timeout=300)
        _REPORTS[seed] = out
    return _REPORTS[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_model_fuzz(gpu, seed):
    out = _run(seed)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "fuzz ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    assert last.startswith(f"fuzz ok: {CASES} random cases compared with the models on the GPU")
    # every component decoded every case on its unlimited tier
    for component, tiers in TIERS.items():
        m = re.search(rf"(?:; ){component} tiers \[([\d, ]*)\] legs (\d+) skipped (\d+)", last)
        assert m, (component, last)
        assert max(tiers) in {int(x) for x in m.group(1).split(",") if x.strip()} and int(m.group(2)) >= CASES


def test_every_tier_of_every_component_ran_over_the_seeds(gpu):
    seen = {c: set() for c in TIERS}
    for seed in SEEDS:
        out = _run(seed)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        for component in TIERS:
            m = re.search(rf"(?:; ){component} tiers \[([\d, ]*)\]", out.stdout.splitlines()[-1])
            seen[component] |= {int(x) for x in m.group(1).split(",") if x.strip()}
    assert seen == TIERS, f"tiers that never ran: { {c: sorted(TIERS[c] - seen[c]) for c in TIERS if TIERS[c] - seen[c]} }"
