"""CPU model of sliding-window decoding: test infrastructure, nothing under ldpcdecoders.jl_amd/ imports it and nothing
here calls the library.  Plain numpy restatements, written from the documents and not from the code: the plan rule of
ldpcdecoders.jl_amd/windows.py's docstring, gather and commit as THE RULE of the ldpc_windows_* section of
include/ldpc_mi355x.h states them, and the chain over the windows around any model decoder.

    window k: layers [a_k, b_k), a_k = k commit, b_k = min(a_k + width, R); the window with b_k = R is the last
    det_k = detectors of those layers; mech_k = mechanisms with a_k <= first(j) < b_k
    commit_k = positions in mech_k with first(j) < a_k + commit (last window: all)
    gather:  win_syndromes(i, r) = residual(i, det_k[r]) & 1
    commit:  guess(i, mech_k[c]) = win_guess(i, c) & 1 for c in commit_k;
             residual(i, d) = (residual(i, d) & 1) ^ XOR of win_guess(i, c) & 1 over the committed c with (d, mech_k[c]) in H,
             for every d with such a c; conv(i) = (k == 0 ? 1 : conv(i) != 0) & (win_conv(i) != 0)
"""
import numpy as np
import scipy.sparse as sp


def _columns(H):
    M = sp.csc_matrix(H)
    M.sort_indices()
    return [[int(d) for d in M.indices[M.indptr[j]:M.indptr[j + 1]]] for j in range(M.shape[1])]


def plan(H, layers, width, commit, strict=True):
    """-> (windows, uncovered): windows = [dict(a, b, det, mech, commit)] with int64 arrays; mechanism by mechanism and
    detector by detector, no vector trick shared with the library."""
    if width < 1 or commit < 1 or commit > width:
        raise ValueError("1 <= commit <= width")
    cols = _columns(H)
    D = sp.csc_matrix(H).shape[0]
    layers = [int(x) for x in layers]
    if len(layers) != D or any(x < 0 for x in layers):
        raise ValueError("layers")
    R = max(layers) + 1 if layers else 0
    first = [min(layers[d] for d in c) if c else None for c in cols]
    last = [max(layers[d] for d in c) if c else None for c in cols]
    windows, k = [], 0
    while R > 0:
        a = k * commit
        b = min(a + width, R)
        is_last = b == R
        det = [d for d in range(D) if a <= layers[d] < b]
        mech = [j for j in range(len(cols)) if first[j] is not None and a <= first[j] < b]
        com = [c for c, j in enumerate(mech) if is_last or first[j] < a + commit]
        if strict and not is_last:
            for c in com:
                j = mech[c]
                if last[j] - first[j] + 1 > width - commit + 1:
                    raise ValueError(f"mechanism {j} would be committed while truncated")
        windows.append(dict(a=a, b=b, det=np.array(det, dtype=np.int64), mech=np.array(mech, dtype=np.int64),
                            commit=np.array(com, dtype=np.int64)))
        if is_last:
            break
        k += 1
    uncovered = np.array([j for j in range(len(cols)) if first[j] is None], dtype=np.int64)
    return windows, uncovered


def sub_matrix(H, window):
    return sp.csc_matrix(sp.csc_matrix(H)[window["det"], :][:, window["mech"]])


def gather(residual, det):
    return (np.asarray(residual)[:, det] & 1).astype(np.uint8)


def commit(H, windows, k, win_guess, residual, guess, win_conv=None, conv=None, want_next=False):
    """In place on residual, guess and conv (numpy uint8); -> the next window's syndromes or None."""
    cols = _columns(H)
    w = windows[k]
    touched = {}
    for c in w["commit"]:
        j = int(w["mech"][c])
        guess[:, j] = win_guess[:, c] & 1
        for d in cols[j]:
            touched.setdefault(d, []).append(int(c))
    for d, cs in touched.items():
        x = residual[:, d] & 1
        for c in cs:
            x = x ^ (win_guess[:, c] & 1)
        residual[:, d] = x
    if win_conv is not None and conv is not None:
        before = np.ones(len(conv), dtype=bool) if k == 0 else conv != 0
        conv[:] = (before & (np.asarray(win_conv) != 0)).astype(np.uint8)
    return gather(residual, windows[k + 1]["det"]) if want_next else None


def chain(H, rates, windows, uncovered, decode_of, syn):
    """The whole decode.  decode_of(H_window, rates_window) -> a function syn [B][s_k] -> (guess [B][n_k], conv [B]).
    -> (errors, conv, residual, stats); stats[k] = dict(unconverged columns of window k, columns whose commit changed the
    next window's syndromes)."""
    syn = np.asarray(syn, dtype=np.uint8)
    B = syn.shape[0]
    rates = np.asarray(rates, dtype=np.float64)
    residual = syn.copy()
    guess = np.full((B, sp.csc_matrix(H).shape[1]), 0xEE, dtype=np.uint8)
    guess[:, uncovered] = 0
    conv = np.ones(B, dtype=np.uint8)
    stats, decoders = [], {}
    wsyn = gather(residual, windows[0]["det"]) if windows else None
    for k, w in enumerate(windows):
        Hw = sub_matrix(H, w)
        key = (Hw.shape, Hw.indptr.tobytes(), Hw.indices.tobytes(), rates[w["mech"]].tobytes())
        if key not in decoders:
            decoders[key] = decode_of(Hw, rates[w["mech"]])
        wg, wc = decoders[key](wsyn)
        wg, wc = np.asarray(wg, dtype=np.uint8), np.asarray(wc, dtype=np.uint8)
        more = k + 1 < len(windows)
        before = gather(residual, windows[k + 1]["det"]) if more else None
        wsyn = commit(H, windows, k, wg, residual, guess, wc, conv, want_next=more)
        stats.append(dict(unconverged=int((wc == 0).sum()), flipped=int((before != wsyn).any(axis=1).sum()) if more else 0))
    stats.append(dict(decoders=len(decoders)))
    return guess, conv, residual, stats
