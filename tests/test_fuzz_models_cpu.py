"""tools/fuzz_models.py without a GPU: the draws of the committed seeds are reproducible, together they contain the shapes
the tool is there for, and the models run a case to the end."""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fuzz_models.py")
CASES, SEEDS = 40, (20, 21)      # what tests/test_gpu_fuzz_models.py runs on the GPU

CASE = re.compile(r"^case (\d+): kind (\d) shape \((\d+), (\d+)\) nnz (\d+) B (\d+) checks<=32 (\d+) checks33-64 (\d+) checks>64 (\d+) "
                  r"empty_checks (\d+) empty_bits (\d+) max_bit_degree (\d+)$")
# the lines of the legs that draw from the second generator; a leg of max_iters 0 decodes nothing and counts for no property
LAYERED = re.compile(r"^   layered .* max_iters (\d+) .* layers (\d+) smallest_layer (\d+) checks<=32 (\d+) checks33-64 (\d+) "
                     r"checks>64 (\d+) checks_empty (\d+)$")
PRIORS = re.compile(r"^   priors (flooding|layered) (floats|given) .* max_iters (\d+) .* nonfinite_rows (\d+)$")
PAULI = re.compile(r"^   pauli Hz \((\d+), (\d+)\) B (\d+) .* max_iters (\d+) .* uniform=(True|False) (sampled|arbitrary) syndromes "
                   r"hx<=32 (\d+) hx33-64 (\d+) hx>64 (\d+) hx_empty (\d+) hz<=32 (\d+) hz33-64 (\d+) hz>64 (\d+) hz_empty (\d+)$")
# the leg of the third generator: the three BP-OTS kernels; S, DC, DV as ldpc_debug_bpots_plan answers for the unforced handle
BPOTS = re.compile(r"^   bpots per (\S+) T (\d+) C (\S+) max_iters (\d+) batch (\d+) (device|host) entry iters=(True|False) "
                   r"edges (\d+) kernel ([235]) S (\d+) DC (\d+) DV (\d+)$")
# the leg of the fourth generator: guided-decimation min-sum; n and the on-chip S of the unforced plan (0: nothing fits) as
# ldpc_debug_decim_tile_plan answers.  A leg of round_iters 0 launches no kernel: it counts for that property alone
DECIM = re.compile(r"^   decim round_iters (\d+) max_decimations (\d+) alpha (\S+) clip (\S+) batch (\d+) (device|host) entry "
                   r"decimated=(True|False) n (\d+) S (\d+)$")
# the leg of the fifth generator: the Pauli relay; a leg whose every count is 0 decodes nothing and counts for no property
PAULI_RELAY = re.compile(r"^   pauli_relay Hz \((\d+), (\d+)\) B (\d+) leg_iters \[([\d, ]+)\] stop_after (\d) negative_gammas (\d+) "
                         r"alpha (\S+) clip (\S+) (device|host) entry llr=(True|False) iters=(True|False) solutions=(True|False) "
                         r"uniform=(True|False) (sampled|arbitrary) syndromes "
                         r"hx<=32 (\d+) hx33-64 (\d+) hx>64 (\d+) hx_empty (\d+) hz<=32 (\d+) hz33-64 (\d+) hz>64 (\d+) hz_empty (\d+)$")
# the leg of the sixth generator: the OSD step by the standard rule
OSD_SEARCH = re.compile(r"^   osd_search (combination_sweep|exhaustive) order (\d+) weights (none|floats|zero|clamped) batch (\d+) "
                        r"reproducing_rows (\d+) nan=(True|False) (in place|out of place)$")
# the leg of the seventh generator: the stabilizer (non-CSS) min-sum; the degrees are those of the union graph
STAB = re.compile(r"^   stab B (\d+) alpha (\S+) clip (\S+) max_iters (\d+) (device|host) entry llr=(True|False) iters=(True|False) "
                  r"uniform=(True|False) (sampled|arbitrary) syndromes x_edges (\d+) z_edges (\d+) y_edges (\d+) "
                  r"checks<=32 (\d+) checks33-64 (\d+) checks>64 (\d+) checks_empty (\d+)$")
OLD_LEGS = ("bitflip", "minsum", "relay", "osd", "trials", "css")
NEW_LEGS = ("layered", "priors", "pauli", "bpots", "decim", "pauli_relay", "osd_search", "stab")
# SHA-256 of a FUZZ_DRY listing of 40 cases without its last line (which carries seconds) and without the lines of the legs
# `pauli_relay`, `osd_search` and `stab`, computed from the tool as it stood before those legs: the eleven older legs draw for a
# committed seed exactly what they drew then
OLDER_LEGS_SHA256 = {20: "79f335c86efda4e16c389aba6c77ae75d485c8f8923acf8f58472b46312e0478", 21: "d0798cff3517aa9a274a5c4bf55af307230cd8ec1dd12ff22a5c4b1b13e2b099"}


def _tool(args, **env):
    out = subprocess.run([sys.executable, TOOL] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600,
                         env={**os.environ, **env})
    assert out.returncode == 0 and "fuzz ok" in out.stdout.splitlines()[-1], out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def coverage(listing):
    """The properties of the issue that the cases of a FUZZ_DRY listing have, as a set of names."""
    have = set()
    for line in listing.splitlines():
        m = LAYERED.match(line)
        if m and int(m.group(1)) > 0:
            _, K, smallest, _, c64, cbig, _ = (int(x) for x in m.groups())
            have |= {name for name, yes in (
                ("layered: check of degree 33 ... 64", c64 > 0), ("layered: check of degree > 64", cbig > 0),
                ("layered: a layer of one check", K > 0 and smallest == 1)) if yes}
        m = PRIORS.match(line)
        if m and int(m.group(3)) > 0:
            have.add(f"priors: {m.group(1)} {m.group(2)}")
            if int(m.group(4)) > 0:
                have.add("priors: a non-finite row")
        m = PAULI.match(line)
        if m and int(m.group(4)) > 0:
            B, uniform, syndromes = int(m.group(3)), m.group(5) == "True", m.group(6)
            _, hx64, hxbig, hxe, _, hz64, hzbig, hze = (int(x) for x in m.groups()[6:])
            have |= {name for name, yes in (
                ("pauli: Hz check of degree 33 ... 64", hz64 > 0), ("pauli: Hz check of degree > 64", hzbig > 0),
                ("pauli: Hx check of degree 33 ... 64", hx64 > 0), ("pauli: Hx check of degree > 64", hxbig > 0),
                ("pauli: empty Hx check", hxe > 0), ("pauli: empty Hz check", hze > 0), ("pauli: batch 1", B == 1),
                ("pauli: batch 65", B == 65), ("pauli: one triple for every qubit", uniform),
                ("pauli: arbitrary syndromes", syndromes == "arbitrary")) if yes}
        m = BPOTS.match(line)
        if m and int(m.group(4)) > 0:
            per, T, kernel, S, DC, DV = float(m.group(1)), int(m.group(2)), int(m.group(9)), int(m.group(10)), int(m.group(11)), int(m.group(12))
            assert int(m.group(5)) <= 65 and (kernel == 2) == (S > 0) and (kernel == 5) == (DC == 0) == (DV == 0)
            have |= {name for name, yes in (
                (f"bpots: S = {S}", kernel == 2), (f"bpots: DC {DC}", kernel == 2), (f"bpots: DV {DV}", kernel == 2),
                ("bpots: T = 1", T == 1), ("bpots: per = 0.75", per == 0.75), ("bpots: a wide graph", kernel == 5),
                ("bpots: a graph without edges", int(m.group(8)) == 0)) if yes}
        m = DECIM.match(line)
        if m:
            T, Dmax, B, n, S = (int(m.group(k)) for k in (1, 2, 5, 8, 9))
            clip, entry, counts = float(m.group(4)), m.group(6), m.group(7) == "True"
            assert 1 <= B <= 65 and 0 <= Dmax <= n and S in (0, 1, 2, 4, 8, 16, 32, 64)
            have |= {name for name, yes in (
                ("decim: round_iters 0", T == 0), ("decim: max_decimations 0", T > 0 and Dmax == 0),
                ("decim: every bit free", T == 1 and Dmax == n > 0), (f"decim: {entry} entry", T > 0),
                ("decim: decimated=False", T > 0 and not counts), (f"decim: clip {clip:g}", T > 0),
                (f"decim: S = {S}", T > 0 and S > 0)) if yes}
        m = PAULI_RELAY.match(line)
        if m and any(int(x) > 0 for x in m.group(4).split(",")):
            B, legs, stop_after, negative = int(m.group(3)), [int(x) for x in m.group(4).split(",")], int(m.group(5)), int(m.group(6))
            assert 1 <= B <= 65 and 1 <= len(legs) <= 4 and max(legs) <= 6 and 1 <= stop_after <= 3
            _, hx64, hxbig, hxe, _, hz64, hzbig, hze = (int(x) for x in m.groups()[14:])
            have |= {name for name, yes in (
                ("pauli_relay: Hx check of degree 33 ... 64", hx64 > 0), ("pauli_relay: Hx check of degree > 64", hxbig > 0),
                ("pauli_relay: Hz check of degree 33 ... 64", hz64 > 0), ("pauli_relay: Hz check of degree > 64", hzbig > 0),
                ("pauli_relay: empty Hx check", hxe > 0), ("pauli_relay: empty Hz check", hze > 0), ("pauli_relay: batch 1", B == 1),
                ("pauli_relay: batch 65", B == 65), ("pauli_relay: a skipped leg", 0 in legs),
                ("pauli_relay: stop_after above 1", stop_after > 1), ("pauli_relay: a negative gamma", negative > 0),
                (f"pauli_relay: {m.group(9)} entry", True), ("pauli_relay: solutions=False", m.group(12) == "False")) if yes}
        m = OSD_SEARCH.match(line)
        if m:
            method, order, kind, B, own = m.group(1), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5))
            assert 1 <= B <= 65 and own <= B and order in ((0, 1, 2, 10, 64) if method == "combination_sweep" else (0, 1, 3, 8))
            have |= {name for name, yes in (
                (f"osd_search: {method}", True), ("osd_search: order 0", order == 0), ("osd_search: order 64", order == 64),
                (f"osd_search: weights {kind}", True), ("osd_search: a row that reproduces its syndrome", own > 0),
                ("osd_search: a NaN LLR", m.group(6) == "True"), ("osd_search: in place", m.group(7) == "in place")) if yes}
        m = STAB.match(line)
        if m and int(m.group(4)) > 0:
            B, clip, entry = int(m.group(1)), float(m.group(3)), m.group(5)
            x, z, y, c32, c64, cbig, ce = (int(v) for v in m.groups()[9:])
            assert 1 <= B <= 65
            have |= {name for name, yes in (
                ("stab: all three edge types", min(x, z, y) > 0), ("stab: check of degree 33 ... 64", c64 > 0),
                ("stab: check of degree > 64", cbig > 0), ("stab: empty check", ce > 0), ("stab: batch 1", B == 1),
                ("stab: batch 65", B == 65), (f"stab: {entry} entry", True), ("stab: llr=False", m.group(6) == "False"),
                ("stab: iters=False", entry == "device" and m.group(7) == "False"), ("stab: one triple for every qubit", m.group(8) == "True"),
                ("stab: arbitrary syndromes", m.group(9) == "arbitrary"), (f"stab: clip {clip:g}", True)) if yes}
        m = CASE.match(line)
        if not m:
            continue
        _, _, s, n, _, B, c32, c64, cbig, ec, eb, bdeg = (int(x) for x in m.groups())
        have |= {name for name, yes in (
            ("check of degree <= 32", c32 > 0), ("check of degree 33 ... 64", c64 > 0), ("check of degree > 64", cbig > 0),
            ("empty check", ec > 0), ("empty bit", eb > 0), ("bit of degree > 64", bdeg > 64), ("n % 64 == 0", n % 64 == 0),
            ("n % 64 == 1", n % 64 == 1), ("n % 64 == 63", n % 64 == 63), ("n % 32 == 1", n % 32 == 1), ("batch 1", B == 1),
            ("batch 65", B == 65)) if yes}
    return have


WANTED = {"check of degree <= 32", "check of degree 33 ... 64", "check of degree > 64", "empty check", "empty bit", "bit of degree > 64",
          "n % 64 == 0", "n % 64 == 1", "n % 64 == 63", "n % 32 == 1", "batch 1", "batch 65",
          "layered: check of degree 33 ... 64", "layered: check of degree > 64", "layered: a layer of one check",
          "priors: flooding floats", "priors: flooding given", "priors: layered floats", "priors: layered given",
          "priors: a non-finite row",
          "pauli: Hz check of degree 33 ... 64", "pauli: Hz check of degree > 64", "pauli: Hx check of degree 33 ... 64",
          "pauli: Hx check of degree > 64", "pauli: empty Hx check", "pauli: empty Hz check", "pauli: batch 1", "pauli: batch 65",
          "pauli: one triple for every qubit", "pauli: arbitrary syndromes",
          # BP-OTS: each register bucket, the bias step in every iteration, a prior of exactly 0, a graph that takes kernel 5 only
          "bpots: DC 8", "bpots: DC 32", "bpots: DV 4", "bpots: DV 16", "bpots: T = 1", "bpots: per = 0.75", "bpots: a wide graph",
          # decimation: no launch, no decimation (plain min-sum), the |D| == n exit, both entries, the optional output left
          # out, the clamp at each of the three clips the leg draws
          "decim: round_iters 0", "decim: max_decimations 0", "decim: every bit free", "decim: device entry", "decim: host entry",
          "decim: decimated=False", "decim: clip 4", "decim: clip 20", "decim: clip 1e+06",
          # Pauli relay, among the legs that run at least one iteration: five-word and per-edge records on each side, an empty
          # check on each side, a one-column and a ragged batch, a leg of 0 iterations next to one that runs, a second and a
          # third solution wanted, a leg that forgets (gamma < 0), both entries, the optional output left out
          "pauli_relay: Hx check of degree 33 ... 64", "pauli_relay: Hx check of degree > 64", "pauli_relay: Hz check of degree 33 ... 64",
          "pauli_relay: Hz check of degree > 64", "pauli_relay: empty Hx check", "pauli_relay: empty Hz check", "pauli_relay: batch 1",
          "pauli_relay: batch 65", "pauli_relay: a skipped leg", "pauli_relay: stop_after above 1", "pauli_relay: a negative gamma",
          "pauli_relay: device entry", "pauli_relay: host entry", "pauli_relay: solutions=False",
          # the standard rule of the OSD step: both methods, no free position (order 0) and more than there are (order 64), each
          # kind of cost, step 1 (bp_err already reproduces the syndrome), the NaN-last order, in place
          "osd_search: combination_sweep", "osd_search: exhaustive", "osd_search: order 0", "osd_search: order 64",
          "osd_search: weights none", "osd_search: weights floats", "osd_search: weights zero", "osd_search: weights clamped",
          "osd_search: a row that reproduces its syndrome", "osd_search: a NaN LLR", "osd_search: in place",
          # stabilizer min-sum, among the legs that run at least one iteration: X-, Z- and Y-type edges in one graph, five-word
          # and per-edge records and an empty check in the union graph, a one-column and a ragged batch, both entries, each
          # optional output left out, the clamp at each of the three clips the leg draws
          "stab: all three edge types", "stab: check of degree 33 ... 64", "stab: check of degree > 64", "stab: empty check",
          "stab: batch 1", "stab: batch 65", "stab: device entry", "stab: host entry", "stab: llr=False", "stab: iters=False",
          "stab: one triple for every qubit", "stab: arbitrary syndromes", "stab: clip 4", "stab: clip 20", "stab: clip 1e+06"}
# A graph without edges is NOT among them: the graphs are the cases' own, drawn from the first generator, whose stream the
# older legs own; the smallest graph of the committed seeds has 7 edges.  tests/test_gpu_bpots_paths.py
# (test_a_graph_without_edges) pins that shape instead.


def test_the_draws_of_a_seed_are_reproducible_and_the_committed_seeds_contain_the_boundary_shapes():
    have = set()
    for seed in SEEDS:
        first = _tool([CASES, seed], FUZZ_DRY="1")
        again = _tool([CASES, seed], FUZZ_DRY="1")
        strip = lambda text: "\n".join(text.splitlines()[:-1])   # noqa: E731  (the last line carries seconds)
        assert strip(first) == strip(again), f"seed {seed}: two dry runs list different cases"
        assert len([ln for ln in first.splitlines() if CASE.match(ln)]) == CASES
        # every leg of every case is listed: the draws do not depend on what ran
        for leg in OLD_LEGS + NEW_LEGS:
            assert len([ln for ln in first.splitlines() if ln.startswith(f"   {leg} ")]) == CASES, leg
        # ... and every line of a new leg is one that coverage() can read
        for leg, pattern in zip(NEW_LEGS, (LAYERED, PRIORS, PAULI, BPOTS, DECIM, PAULI_RELAY, OSD_SEARCH, STAB)):
            assert all(pattern.match(ln) for ln in first.splitlines() if ln.startswith(f"   {leg} ")), leg
        # ... and the eleven older legs draw what they drew before the legs pauli_relay, osd_search and stab existed
        older = [ln for ln in first.splitlines()[:-1] if not ln.startswith(("   pauli_relay ", "   osd_search ", "   stab "))]
        assert hashlib.sha256(("\n".join(older) + "\n").encode()).hexdigest() == OLDER_LEGS_SHA256[seed], f"seed {seed}: an older leg draws otherwise"
        have |= coverage(first)
    widths = {name for name in have if name.startswith("bpots: S = ")}
    assert len(widths) >= 3, f"the committed seeds reach only the BP-OTS tile widths {sorted(widths)}"
    assert "bpots: a graph without edges" not in have       # (see WANTED: if a seed ever draws one, say so there)
    decim_widths = {name for name in have if name.startswith("decim: S = ")}
    assert len(decim_widths) >= 3, f"the committed seeds reach only the decimation tile widths {sorted(decim_widths)}"
    assert have - widths - decim_widths == WANTED, f"the committed seeds never draw: {sorted(WANTED - have)}"


def test_a_window_of_cases_draws_what_the_whole_run_draws():
    """FUZZ_FROM / FUZZ_TO skip cases without changing the later draws."""
    whole = _tool([6, SEEDS[0]], FUZZ_DRY="1", FUZZ_VERBOSE="1")
    window = _tool([6, SEEDS[0]], FUZZ_MODEL_ONLY="1", FUZZ_VERBOSE="1", FUZZ_FROM="4", FUZZ_TO="4")
    listed = lambda text: [ln for ln in text.splitlines() if ln.startswith(("case ", "   "))]   # noqa: E731
    assert listed(whole) == listed(window)


def test_one_case_runs_through_the_models_to_the_end():
    out = _tool([3, SEEDS[0]], FUZZ_MODEL_ONLY="1", FUZZ_FROM="2", FUZZ_TO="2")
    assert "model seconds: bitflip" in out and "through the models only" in out.splitlines()[-1]
    assert all(f"{leg} " in out.splitlines()[-2] for leg in OLD_LEGS + NEW_LEGS)
