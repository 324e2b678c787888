"""CPU model of the rule the device form of the OSD step states (include/ldpc_mi355x.h, csrc/osd_kernels.hpp):
key = max(p, 1-p) with p = pm_exp(llr) (csrc/portable_math.h), columns ordered by (key descending, column index
ascending), a NaN key last.

It leans on the independent dense oracle (oracle/osd_oracle.c) instead of a third elimination: the columns are
grouped into tie classes in that order, and the oracle is handed SURROGATE LLRs that realise exactly that order and
those ties under any exp -- one well separated value per tie class, log(0.5 + 0.4 (K - class) / K) for K classes:
equal inputs give equal keys, and the keys of two classes are >= 0.4 / n apart.
"""
import math

import numpy as np

from oracle import osd_oracle_postprocess

_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
_INV_LN2 = 1.44269504088896338700e+00


def pm_exp(x):
    """portable_math.h pm_exp restated in numpy float64: only + - * /, trunc and ldexp, each correctly rounded or
    exact, in the same order -- bit-identical to the C function compiled with -ffp-contract=off."""
    x = np.asarray(x, dtype=np.float64)
    nan, big, small = np.isnan(x), x > 709.0, x < -708.0
    xs = np.where(nan | big | small, 0.0, x)
    t = xs * _INV_LN2
    k = np.trunc(np.where(t < 0.0, t - 0.5, t + 0.5))
    r = (xs - k * _LN2_HI) - k * _LN2_LO
    p = 1.0 + r * (1.0 / 14.0)
    for d in (13.0, 12.0, 11.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0):
        p = 1.0 + (r * p) * (1.0 / d)
    p = 1.0 + r * p
    out = p * np.ldexp(1.0, k.astype(np.int64))
    out = np.where(big, np.inf, out)
    out = np.where(small, 0.0, out)
    return np.where(nan, x, out)


def key_bits(llr):
    """The keys as the device compares them: the bit pattern of max(p, 1-p) (doubles >= 0.5 order like unsigned
    integers), 0 for a NaN."""
    with np.errstate(invalid="ignore"):
        p = pm_exp(llr)
        q = 1.0 - p
        k = np.where(p > q, p, q)
    bits = np.ascontiguousarray(k, dtype=np.float64).view(np.uint64).copy()
    bits[np.isnan(k)] = 0
    return bits


def model_order(llr):
    """Column order of the rule: (key descending, index ascending); and the tie class of each sorted position."""
    bits = key_bits(np.asarray(llr, dtype=np.float64).reshape(-1))
    perm = np.argsort(~bits, kind="stable")
    sb = bits[perm]
    cls = np.zeros(perm.size, dtype=np.int64)
    if perm.size:
        cls[1:] = np.cumsum(sb[1:] != sb[:-1])
    return perm, cls


def libm_order(llr):
    """The host form's order: key from libm's exp (math.exp), stable descending sort."""
    key = np.empty(len(llr), dtype=np.float64)
    for j, v in enumerate(np.asarray(llr, dtype=np.float64)):
        try:
            p = math.exp(v)
        except OverflowError:
            p = math.inf
        q = 1.0 - p
        key[j] = p if p > q else q
    # std::stable_sort with `a > b`: stable, descending (no NaN on the workloads this is used for)
    return np.argsort(-key, kind="stable")


def surrogate_llr(llr):
    """LLRs whose libm keys realise the model's order and ties."""
    perm, cls = model_order(llr)
    K = int(cls[-1]) + 1 if perm.size else 1
    out = np.empty(perm.size, dtype=np.float64)
    out[perm] = np.log(0.5 + 0.4 * (K - cls) / K)
    return out


def osd_model_postprocess(Hd, syndrome, bp_err, llr, osd_order):
    """The estimate the device form must return for ONE syndrome (a syndrome entry that is not 0 counts as 1)."""
    syn = (np.asarray(syndrome) != 0).astype(np.uint8)
    return osd_oracle_postprocess(Hd, syn, bp_err, surrogate_llr(llr), osd_order)
