"""Detector error models on the host (numpy / scipy, no library call of its own): what a decoder of measurement noise
is given -- a detector check matrix `H` (detectors x mechanisms), an observables matrix `L` (observables x mechanisms)
and one probability per error mechanism -- with the usual line-oriented text form, the phenomenological model
(repeated noisy measurement) of any check matrix, and `run_dem_trials`, which is `run_trials` at per-bit rates:
mechanism j is bit j of the sampler (`Trials.set_rates` / `sample_rates`), the detectors are its syndrome, and a
logical failure is `L * (guess ^ error) != 0`."""
from __future__ import annotations

import re
from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp

from .decoder import _pattern_of

_INSTRUCTION = re.compile(r"^([A-Za-z_][A-Za-z_0-9]*)\s*(?:\(([^()]*)\))?\s*(.*)$")
_TARGET = re.compile(r"^([DL])(\d+)$")


def _columns_matrix(columns: List[Tuple[int, ...]], rows: int) -> sp.csc_matrix:
    """The `rows` x len(columns) pattern whose column j holds the (ascending, distinct) rows columns[j]."""
    indptr = np.zeros(len(columns) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in columns], out=indptr[1:])
    indices = np.fromiter((r for c in columns for r in c), dtype=np.int64, count=int(indptr[-1]))
    return sp.csc_matrix((np.ones(indices.size, dtype=np.uint8), indices, indptr), shape=(rows, len(columns)))


class DetectorErrorModel:
    """`H` detectors x mechanisms, `L` observables x mechanisms (0 rows are fine), `rates` one probability in [0, 1] per
    mechanism.  Stored as CSC patterns (`.H`, `.L`) and a float64 array (`.rates`)."""

    def __init__(self, H, L, rates):
        self.H = _pattern_of(H)
        n = int(self.H.shape[1])
        self.L = sp.csc_matrix((0, n), dtype=np.uint8) if L is None else _pattern_of(L)
        if int(self.L.shape[1]) != n:
            raise ValueError("L must have as many columns (mechanisms) as H")
        self.rates = np.array(rates, dtype=np.float64).reshape(-1)
        if self.rates.shape != (n,):
            raise ValueError(f"one rate per mechanism: expected {n} entries, got {self.rates.size}")
        if n and not np.all((self.rates >= 0.0) & (self.rates <= 1.0)):   # (False for NaN as well)
            raise ValueError("rates must lie in [0, 1]")

    @property
    def num_detectors(self) -> int:
        return int(self.H.shape[0])

    @property
    def num_observables(self) -> int:
        return int(self.L.shape[0])

    @property
    def num_mechanisms(self) -> int:
        return int(self.H.shape[1])

    @property
    def channel_probs(self) -> np.ndarray:
        """The priors of a decoder with one per bit (`MinSumDecoder(dem.H, None, iters, channel_probs=...)`)."""
        return self.rates

    def trials(self, device: Optional[int] = None):
        """A `Trials(H, L)` on `device` with the rates set."""
        from .trials import Trials

        t = Trials(self.H, self.L, device=device)
        t.set_rates(self.rates)
        return t

    def __eq__(self, other) -> bool:
        if not isinstance(other, DetectorErrorModel):
            return NotImplemented
        return (self.H.shape == other.H.shape and self.L.shape == other.L.shape and (self.H != other.H).nnz == 0
                and (self.L != other.L).nnz == 0 and np.array_equal(self.rates, other.rates))

    __hash__ = None

    # -- the text form ---------------------------------------------------------------------------------------------
    def to_text(self) -> str:
        """One `error(p) D.. L..` line per mechanism, `p` printed with `repr` (so reading it back is exact), and a
        declaration of the last detector / observable where no mechanism names it.  `from_text` of the result is this
        model again as long as no two mechanisms have the same effect and none has an empty one (those are merged /
        dropped on reading)."""
        lines = []
        Hp, Hi, Lp, Li = self.H.indptr, self.H.indices, self.L.indptr, self.L.indices
        for j in range(self.num_mechanisms):
            targets = [f"D{int(d)}" for d in Hi[Hp[j]:Hp[j + 1]]] + [f"L{int(o)}" for o in Li[Lp[j]:Lp[j + 1]]]
            lines.append(f"error({float(self.rates[j])!r}) " + " ".join(targets))
        if self.num_detectors and (self.H.nnz == 0 or int(Hi.max()) != self.num_detectors - 1):
            lines.append(f"detector D{self.num_detectors - 1}")
        if self.num_observables and (self.L.nnz == 0 or int(Li.max()) != self.num_observables - 1):
            lines.append(f"logical_observable L{self.num_observables - 1}")
        return "\n".join(lines) + "\n"

    @classmethod
    def from_text(cls, text: str) -> "DetectorErrorModel":
        """Reads `error(p) D3 D7 L0` lines (`^` separators are ignored; the effect of a mechanism is the XOR of all its
        targets, so a target named twice cancels), `detector...` and `logical_observable...` declarations (they only extend
        the counts), `shift_detectors(...) k`, nested `repeat N { ... }` blocks and `#` comments.  Mechanisms with an
        identical effect are merged (`p = p1 + p2 - 2 p1 p2`, in order of appearance) and one with an empty effect is
        dropped.  A malformed line is a ValueError that names its line number."""
        program = _parse_block(_tokenise(text), [0], None)
        state = {"shift": 0, "detectors": 0, "observables": 0, "order": [], "p": {}}
        _run_block(program, state)
        order = state["order"]
        H = _columns_matrix([dets for dets, _ in order], state["detectors"])
        L = _columns_matrix([obs for _, obs in order], state["observables"])
        return cls(H, L, [state["p"][k] for k in order])


def _tokenise(text: str):
    """-> [(line number, instruction name, arguments in parentheses or None, the rest)] of the non-empty lines; a
    closing brace is the name '}', an opening one ends the rest of a `repeat` line."""
    out = []
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        if line == "}":
            out.append((no, "}", None, ""))
            continue
        m = _INSTRUCTION.match(line)
        if not m:
            raise ValueError(f"line {no}: cannot read {raw.strip()!r}")
        out.append((no, m.group(1), m.group(2), m.group(3).strip()))
    return out


def _parse_block(tokens, at, opened_at):
    """The instructions from tokens[at[0]] up to the closing brace of the block opened in line `opened_at` (None: the
    whole text); a `repeat` holds its own block."""
    block = []
    while at[0] < len(tokens):
        no, name, args, rest = tokens[at[0]]
        at[0] += 1
        if name == "}":
            if opened_at is None:
                raise ValueError(f"line {no}: '}}' without a repeat block")
            return block
        if name == "repeat":
            parts = rest.split()
            if args is not None or len(parts) != 2 or parts[1] != "{" or not parts[0].isdigit():
                raise ValueError(f"line {no}: a repeat block starts with 'repeat N {{'")
            block.append((no, name, int(parts[0]), _parse_block(tokens, at, no)))
        elif name in ("error", "detector", "logical_observable", "shift_detectors"):
            if "{" in rest or "}" in rest:
                raise ValueError(f"line {no}: a brace inside a {name} instruction")
            block.append((no, name, args, rest))
        else:
            raise ValueError(f"line {no}: unknown instruction {name!r}")
    if opened_at is not None:
        raise ValueError(f"line {opened_at}: the repeat block is never closed")
    return block


def _targets(no: int, rest: str, shift: int):
    """-> (detectors, observables, detector count, observable count): the targets named an odd number of times
    (detectors absolute), and the counts that all named targets imply."""
    dets, obs, nd, nobs = set(), set(), 0, 0
    for word in rest.split():
        if word == "^":
            continue
        m = _TARGET.match(word)
        if not m:
            raise ValueError(f"line {no}: {word!r} is no target (D<number>, L<number> or ^)")
        k = int(m.group(2))
        if m.group(1) == "D":
            k += shift
            dets ^= {k}
            nd = max(nd, k + 1)
        else:
            obs ^= {k}
            nobs = max(nobs, k + 1)
    return dets, obs, nd, nobs


def _run_block(block, state) -> None:
    for no, name, args, rest in block:
        if name == "repeat":
            for _ in range(args):
                _run_block(rest, state)
            continue
        if name == "shift_detectors":
            if not rest.isdigit():
                raise ValueError(f"line {no}: shift_detectors takes one non-negative whole number")
            state["shift"] += int(rest)
            continue
        dets, obs, nd, nobs = _targets(no, rest, state["shift"])
        state["detectors"] = max(state["detectors"], nd)
        state["observables"] = max(state["observables"], nobs)
        if name != "error":
            continue                                       # a declaration: the counts only
        try:
            p = float(args)
        except (TypeError, ValueError):
            raise ValueError(f"line {no}: error(p) needs one probability") from None
        if not 0.0 <= p <= 1.0:                            # (False for NaN as well)
            raise ValueError(f"line {no}: the probability {args.strip()} lies outside [0, 1]")
        key = (tuple(sorted(dets)), tuple(sorted(obs)))
        if not key[0] and not key[1]:
            continue                                       # no effect
        if key in state["p"]:
            q = state["p"][key]
            state["p"][key] = q + p - 2.0 * q * p
        else:
            state["order"].append(key)
            state["p"][key] = p


def phenomenological(H, logicals, rounds: int, p, q) -> DetectorErrorModel:
    """The phenomenological model of check matrix `H` (s x n) over `rounds` = R >= 1 rounds of syndrome extraction, the
    last one measured perfectly.  Detector (t, i) (row t s + i) is check i of round t XOR check i of round t - 1 (round
    -1: all zero).  Mechanisms, in column order: a data error on bit j entering before round t, t = 0 ... R - 1
    (round-major, rate p), flips the detectors (t, i) of the checks i of j and the observables of j; then a measurement
    error of check i in round t, t = 0 ... R - 2 (rate q), flips the detectors (t, i) and (t + 1, i) and no observable.
    So H_dem = [I_R (x) H | D (x) I_s] with D the R x (R - 1) lower bidiagonal: R n + (R - 1) s mechanisms, R s
    detectors.  `p` / `q`: a scalar, or one rate per bit / per check."""
    R = int(rounds)
    if R < 1:
        raise ValueError("rounds must be >= 1")
    M = _pattern_of(H)
    s, n = int(M.shape[0]), int(M.shape[1])
    Lm = sp.csc_matrix((0, n), dtype=np.uint8) if logicals is None else _pattern_of(logicals)
    if int(Lm.shape[1]) != n:
        raise ValueError("logicals must have as many columns as H")
    pj = np.broadcast_to(np.asarray(p, dtype=np.float64), (n,))
    qi = np.broadcast_to(np.asarray(q, dtype=np.float64), (s,))
    D = sp.diags([np.ones(R - 1), np.ones(R - 1)], [0, -1], shape=(R, R - 1), dtype=np.uint8) if R > 1 else sp.csc_matrix((1, 0), dtype=np.uint8)
    H_dem = sp.hstack([sp.kron(sp.identity(R, dtype=np.uint8), M), sp.kron(D, sp.identity(s, dtype=np.uint8))], format="csc")
    L_dem = sp.hstack([sp.hstack([Lm] * R), sp.csc_matrix((int(Lm.shape[0]), (R - 1) * s), dtype=np.uint8)], format="csc")
    return DetectorErrorModel(H_dem, L_dem, np.concatenate([np.tile(pj, R), np.tile(qi, R - 1)]))


def run_dem_trials(dem: DetectorErrorModel, decoder, trials: int, batch: int = 65536, seed: int = 0):
    """`run_trials(decoder, trials, per=dem.rates, logicals=dem.L)` after checking that the decoder decodes `dem.H`: every
    mechanism is drawn at its own rate, the decoder sees the detectors, the score counts the observables it gets wrong.
    Any decoder that `run_trials` drives; for `MinSumDecoder` / `RelayMinSumDecoder` the natural construction is
    `channel_probs=dem.rates`."""
    from .osd import BeliefPropagationOSDDecoder
    from .trials import run_trials

    bp = decoder.bp_decoder if isinstance(decoder, BeliefPropagationOSDDecoder) else decoder
    Hd = _pattern_of(bp.sparse_H)
    if Hd.shape != dem.H.shape or (Hd != dem.H).nnz != 0:
        raise ValueError("the decoder's check matrix is not the detector error model's H")
    return run_trials(decoder, trials, per=dem.rates, batch=batch, seed=seed, logicals=dem.L)
