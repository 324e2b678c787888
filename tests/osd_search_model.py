"""The standard rule of the OSD step (include/ldpc_mi355x.h, "THE STANDARD RULE"; csrc/osd_search_kernels.hpp) in
numpy: dense GF(2) Gauss-Jordan elimination with row swaps, the candidate enumeration written out, int64 costs.  Every
step is integer arithmetic or an exact comparison of doubles, so the device must equal this in every element."""
import numpy as np

EXHAUSTIVE, SWEEP = 1, 2
METHODS = {"exhaustive": EXHAUSTIVE, "combination_sweep": SWEEP}


def weights_of(channel_llr):
    """q[j] = (int64) rint(clamp(channel_llr[j], -2^24, 2^24) * 2^16), ties to even: the relay decoder's formula."""
    x = np.clip(np.asarray(channel_llr, dtype=np.float64), -16777216.0, 16777216.0)
    return np.rint(x * 65536.0).astype(np.int64)


def search_order(llr):
    """Ascending llr, ties by ascending index, -0.0 = +0.0, a NaN last (numpy's sort order), NaNs by index."""
    x = np.asarray(llr, dtype=np.float64).reshape(-1)
    return np.argsort(np.where(x == 0.0, 0.0, x), kind="stable")


def eliminate(Hd, syn, perm):
    """Gauss-Jordan over the columns in the order `perm`.  Returns (pivot columns in pivot-row order, non-pivot columns
    t_0 .. t_{K-1}, R = the reduced r pivot rows over the original columns [r][n], sr = their syndrome bits [r])."""
    m, n = Hd.shape
    A = np.packbits(np.concatenate([Hd.astype(np.uint8), (np.asarray(syn) != 0).astype(np.uint8).reshape(m, 1)], axis=1), axis=1)
    piv, r = [], 0
    for c in perm:
        if r >= m:
            break
        byte, bit = int(c) >> 3, 0x80 >> (int(c) & 7)
        has = (A[:, byte] & bit) != 0
        cand = np.nonzero(has[r:])[0]
        if cand.size == 0:
            continue
        i = r + int(cand[0])
        if i != r:
            A[[r, i]] = A[[i, r]]
            has[[r, i]] = has[[i, r]]
        has[r] = False
        A[has] ^= A[r]
        piv.append(int(c))
        r += 1
    full = np.unpackbits(A[:r], axis=1)[:, :n + 1]
    is_piv = np.zeros(n, dtype=bool)
    is_piv[piv] = True
    nonpiv = np.array([int(c) for c in perm if not is_piv[c]], dtype=np.int64)
    return np.array(piv, dtype=np.int64), nonpiv, full[:, :n], full[:, n]


def candidates(method, order, K):
    """The sets F as tuples of positions into t, in the rule's enumeration."""
    w = min(int(order), int(K))
    if method == EXHAUSTIVE:
        return [tuple(k for k in range(w) if (x >> k) & 1) for x in range(1 << w)]
    out = [()] + [(k,) for k in range(K)]
    out += [(a, b) for a in range(w) for b in range(a + 1, w)]
    return out


def osd_search_model(Hd, syn, bp_err, llr, method, order, q=None, want_cost=False):
    """The estimate for ONE syndrome.  q: int64 weights (None: all 1)."""
    Hd = np.asarray(Hd, dtype=np.uint8)
    m, n = Hd.shape
    s = (np.asarray(syn) != 0).astype(np.uint8)
    bp = (np.asarray(bp_err) == 1).astype(np.uint8)
    q = np.ones(n, dtype=np.int64) if q is None else np.asarray(q, dtype=np.int64)
    if np.array_equal((Hd.astype(np.int64) @ bp.astype(np.int64)) % 2, s):          # step 1
        return (bp, int((bp.astype(np.int64) * q).sum())) if want_cost else bp
    piv, t, R, sr = eliminate(Hd, s, search_order(llr))
    K, w = t.size, min(int(order), int(t.size))
    qp, qt = q[piv], q[t]
    cols = R[:, t].T.astype(np.uint8)                                                # [K][r]: column t_k over the pivot rows
    if method == EXHAUSTIVE:
        X = ((np.arange(1 << w)[:, None] >> np.arange(w)[None, :]) & 1).astype(np.float64)   # [2^w][w]
        P = (np.rint(X @ cols[:w].astype(np.float64)).astype(np.int64) + sr[None, :]) & 1
        cost = P @ qp + X.astype(np.int64) @ qt[:w]
        best = int(np.argmin(cost))                                                  # the first minimum: lowest index
        F = [k for k in range(w) if (best >> k) & 1]
    else:
        pa, pb = np.triu_indices(w, 1)                                               # a ascending, then b ascending
        P = np.concatenate([sr[None, :], cols ^ sr[None, :], cols[pa] ^ cols[pb] ^ sr[None, :]], axis=0).astype(np.int64)
        own = np.concatenate([[0], qt, qt[pa] + qt[pb]]).astype(np.int64)
        cost = P @ qp + own
        best = int(np.argmin(cost))
        F = [] if best == 0 else [best - 1] if best <= K else [int(pa[best - 1 - K]), int(pb[best - 1 - K])]
    e = np.zeros(n, dtype=np.uint8)
    e[t[np.array(F, dtype=np.int64)]] = 1
    e[piv] = P[best]
    return (e, int(cost[best])) if want_cost else e
