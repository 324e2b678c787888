"""Input side of the hot path: parity-check matrices and synthetic workloads.

    parity_check_matrix(n, wr, wc)   src/parity_generator.jl:21-45  (Gallager regular LDPC)
    save_pcm / load_pcm              src/parity_generator.jl:47-54

The reference draws its column shuffles from Julia's unseeded global RNG
(:41), so its matrices are not reproducible; this generator keeps the same
*structure* (block 0 = consecutive runs of ``wr`` ones, blocks 1..wc-1 = column
permutations of block 0) with a documented, seeded PRNG: splitmix64 driving a
Fisher-Yates shuffle, seed = ``seed + block index``.

Pure host code (numpy); nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import scipy.sparse as sp

DEFAULT_SEED = 0x4C445043  # "LDPC"
_M64 = (1 << 64) - 1


class SplitMix64:
    """splitmix64 (Steele, Lea, Flood 2014); the documented PRNG of this package."""

    def __init__(self, seed: int):
        self.x = seed & _M64

    def next(self) -> int:
        self.x = (self.x + 0x9E3779B97F4A7C15) & _M64
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)


def shuffled_indices(n: int, seed: int) -> np.ndarray:
    """Fisher-Yates permutation of 0..n-1 (stands in for `shuffle(1:end)`, parity_generator.jl:41)."""
    rng = SplitMix64(seed)
    p = list(range(n))
    for i in range(n - 1, 0, -1):
        j = rng.next() % (i + 1)
        p[i], p[j] = p[j], p[i]
    return np.asarray(p, dtype=np.int64)


def parity_check_csc(n: int, wr: int, wc: int, seed: int = DEFAULT_SEED) -> sp.csc_matrix:
    """Gallager (wc, wr)-regular parity-check matrix as a sparse ``(n*wc/wr) x n`` pattern.

    Block b, column c has its single one in row ``b*block_size + perm_b[c] // wr``
    where perm_0 is the identity (parity_generator.jl:32-42: ``block[:, shuffle(1:end)]``
    puts old column ``perm[c]`` at position ``c``)."""
    if n % wr != 0:
        raise AssertionError("n % wr == 0")  # parity_generator.jl:25
    n_equations = (n * wc) // wr
    block_size = n_equations // wc
    rows = np.empty((wc, n), dtype=np.int64)
    rows[0] = np.arange(n) // wr
    for b in range(1, wc):
        perm = shuffled_indices(n, seed + b)
        rows[b] = b * block_size + perm // wr
    indices = rows.T.reshape(-1)               # column-major: per bit, blocks (= rows) ascending
    indptr = np.arange(0, n * wc + 1, wc, dtype=np.int64)
    data = np.ones(n * wc, dtype=np.bool_)
    return sp.csc_matrix((data, indices, indptr), shape=(n_equations, n))


def parity_check_matrix(n: int, wr: int, wc: int, seed: int = DEFAULT_SEED) -> np.ndarray:
    """`parity_check_matrix(n, wr, wc)` (parity_generator.jl:21-45) as a dense bool matrix
    (the reference returns a BitMatrix)."""
    return np.asarray(parity_check_csc(n, wr, wc, seed).todense()).astype(np.bool_)


def save_pcm(H, file_path) -> None:
    """`save_pcm(H, file_path)` (parity_generator.jl:47-49): `writedlm(file_path, Int.(H))`,
    i.e. tab-delimited 0/1 rows."""
    A = np.asarray(H.todense() if sp.issparse(H) else H).astype(np.int64)
    with open(file_path, "w") as f:
        for row in A:
            f.write("\t".join(str(int(v)) for v in row) + "\n")


def load_pcm(file_path) -> np.ndarray:
    """`load_pcm(file_path)` (parity_generator.jl:51-54): `Int.(readdlm(file_path))`."""
    rows = []
    with open(file_path) as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([int(float(t)) for t in line.replace(",", " ").split()])
    return np.asarray(rows, dtype=np.int64)


def bivariate_bicycle_72_12_6() -> Tuple[np.ndarray, np.ndarray]:
    """[[72,12,6]] bivariate-bicycle code (BASELINE config 5; not in the reference).

    l = m = 6, x = S_6 (x) I_6, y = I_6 (x) S_6, A = x^3 + y + y^2, B = y^3 + x + x^2,
    H_X = [A | B], H_Z = [B' | A'].  Returns (H_X, H_Z), each 36 x 72, row weight 6."""
    ell = m = 6
    S_l = np.roll(np.eye(ell, dtype=np.int64), 1, axis=1)
    S_m = np.roll(np.eye(m, dtype=np.int64), 1, axis=1)
    x = np.kron(S_l, np.eye(m, dtype=np.int64))
    y = np.kron(np.eye(ell, dtype=np.int64), S_m)
    mp = np.linalg.matrix_power
    A = (mp(x, 3) + y + mp(y, 2)) % 2
    B = (mp(y, 3) + x + mp(x, 2)) % 2
    HX = np.concatenate([A, B], axis=1) % 2
    HZ = np.concatenate([B.T, A.T], axis=1) % 2
    return HX.astype(np.bool_), HZ.astype(np.bool_)


def random_errors(n: int, batch: int, per: float, seed: int) -> np.ndarray:
    """i.i.d. Bernoulli(per) error patterns, [batch][n] uint8 (numpy PCG64, seeded)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.random((batch, n)) < per).astype(np.uint8)


def syndromes_of(H, errors_bn: np.ndarray) -> np.ndarray:
    """syndrome = (H * e) .% 2 for every row of errors [B][n]; returns [B][s] uint8."""
    M = sp.csr_matrix(H, dtype=np.int32) if not sp.issparse(H) else sp.csr_matrix(H.astype(np.int32))
    return (np.asarray((M @ errors_bn.T.astype(np.int32))) % 2).T.astype(np.uint8).copy()


# ---- CSS codes: a product family and the logical operators (host GF(2) elimination; run once per code) --------------
def _dense_bits(H) -> np.ndarray:
    """The pattern of H (its nonzero entries, as the decoders take it) as a dense 0/1 uint8 matrix."""
    A = np.asarray(H.todense()) if sp.issparse(H) else np.asarray(H)
    return (A != 0).astype(np.uint8)


def _gf2_rref(A: np.ndarray):
    """Reduced row echelon form over GF(2) of a dense 0/1 matrix -> (R [rank][n] uint8, pivot columns).  The rows are
    eliminated bit-packed (numpy.packbits), one XOR of whole rows per pivot."""
    r, n = A.shape
    P = np.packbits(A, axis=1) if n else np.zeros((r, 0), dtype=np.uint8)
    pivots, rank = [], 0
    for c in range(n):
        if rank == r:
            break
        byte, mask = c >> 3, 0x80 >> (c & 7)
        hit = np.nonzero(P[rank:, byte] & mask)[0]
        if hit.size == 0:
            continue
        p = rank + int(hit[0])
        if p != rank:
            P[[rank, p]] = P[[p, rank]]
        rows = np.nonzero(P[:, byte] & mask)[0]
        rows = rows[rows != rank]
        P[rows] ^= P[rank]
        pivots.append(c)
        rank += 1
    R = np.unpackbits(P[:rank], axis=1, count=n) if n else np.zeros((rank, 0), dtype=np.uint8)
    return R, pivots


def gf2_rank(A) -> int:
    """Rank over GF(2)."""
    return len(_gf2_rref(_dense_bits(A))[1])


def _gf2_kernel(A: np.ndarray) -> np.ndarray:
    """A basis (rows) of {v : A v = 0} over GF(2)."""
    n = A.shape[1]
    R, pivots = _gf2_rref(A)
    free = np.setdiff1d(np.arange(n), np.asarray(pivots, dtype=np.int64))
    K = np.zeros((free.size, n), dtype=np.uint8)
    K[np.arange(free.size), free] = 1
    if pivots:
        K[:, pivots] = R[:, free].T
    return K


def _first_independent_rows(S: np.ndarray) -> list:
    """Indices of the rows of S that are independent of the rows before them (the pivot columns of S')."""
    return _gf2_rref(np.ascontiguousarray(S.T))[1]


def _gf2_matmul(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A * B over GF(2) for 0/1 matrices (float32 products are exact: the inner dimension is far below 2^24)."""
    assert A.shape[1] < (1 << 24)
    return (np.rint(A.astype(np.float32) @ B.astype(np.float32)).astype(np.int64) & 1).astype(np.uint8)


def _gf2_inverse(M: np.ndarray) -> np.ndarray:
    k = M.shape[0]
    R, pivots = _gf2_rref(np.concatenate([M, np.eye(k, dtype=np.uint8)], axis=1))
    if pivots != list(range(k)):
        raise AssertionError("matrix is singular over GF(2)")
    return R[:, k:]


def css_logicals(Hx, Hz) -> Tuple[np.ndarray, np.ndarray]:
    """Logical operators of the CSS code (Hx, Hz), Hx * Hz' = 0 over GF(2): -> (Lx, Lz), each k x n uint8 with
    k = n - rank(Hx) - rank(Hz).  The rows of Lx span ker(Hz) modulo rowspace(Hx), those of Lz span ker(Hx) modulo
    rowspace(Hz), and they are paired: Lx * Lz' = I_k.  Host elimination in numpy, for create time."""
    X, Z = _dense_bits(Hx), _dense_bits(Hz)
    if X.shape[1] != Z.shape[1]:
        raise AssertionError("Hx and Hz must have the same number of columns")
    if _gf2_matmul(X, Z.T).any():
        raise AssertionError("Hx * Hz' != 0 over GF(2): not a CSS code")

    def quotient(H_kernel_of, H_modulo):
        K = _gf2_kernel(H_kernel_of)
        R, pivots = _gf2_rref(H_modulo)
        if pivots:
            K = K ^ _gf2_matmul(K[:, pivots], R)   # every row reduced modulo rowspace(H_modulo): zero in its pivot columns
        return K[_first_independent_rows(K)]

    Lx, Lz = quotient(Z, X), quotient(X, Z)
    k = Lx.shape[0]
    if Lz.shape[0] != k:
        raise AssertionError("logical X and Z spaces differ in dimension")
    if k:
        # Lz <- inv(M)' * Lz with M = Lx * Lz', so that Lx * Lz' = M * inv(M) = I
        Lz = _gf2_matmul(np.ascontiguousarray(_gf2_inverse(_gf2_matmul(Lx, Lz.T)).T), Lz)
    return Lx, Lz


def hypergraph_product(H1, H2=None) -> Tuple[sp.csc_matrix, sp.csc_matrix]:
    """Hypergraph product (Tillich, Zemor 2014) of two classical parity-check matrices H1 (m1 x n1) and H2 (m2 x n2,
    default H1): Hx = [H1 (x) I_n2 | I_m1 (x) H2'] (m1 n2 rows), Hz = [I_n1 (x) H2 | H1' (x) I_m2] (n1 m2 rows), on
    n1 n2 + m1 m2 qubits; Hx * Hz' = 2 (H1 (x) H2') = 0 over GF(2).  Sparse uint8 patterns."""
    A = sp.csr_matrix(_dense_bits(H1))
    B = A if H2 is None else sp.csr_matrix(_dense_bits(H2))
    (m1, n1), (m2, n2) = A.shape, B.shape
    eye = lambda k: sp.identity(k, dtype=np.uint8, format="csr")   # noqa: E731
    Hx = sp.hstack([sp.kron(A, eye(n2)), sp.kron(eye(m1), B.T)])
    Hz = sp.hstack([sp.kron(eye(n1), B), sp.kron(A.T, eye(m2))])
    out = []
    for M in (Hx, Hz):
        M = sp.csc_matrix(M).astype(np.uint8)
        M.sum_duplicates()
        M.eliminate_zeros()   # (kron stores the zeros of a dense block)
        M.sort_indices()
        out.append(M)
    return out[0], out[1]


# ---- general stabilizer codes: the symplectic pair (Sx, Sz), Clifford deformation, logical operators ----------------
# A stabilizer with X or Y on qubit j has Sx[i, j] = 1, with Z or Y it has Sz[i, j] = 1.  The symplectic product of two
# Paulis (x1 | z1), (x2 | z2) is x1 . z2 + z1 . x2 over GF(2): 1 where they anticommute.
PAULI_PERMUTATIONS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")   # the images of X, Y, Z under a single-qubit Clifford


def paulis_to_symplectic(strings) -> Tuple[np.ndarray, np.ndarray]:
    """Pauli strings over I, X, Y, Z (one per stabilizer, all of one length) -> (Sx, Sz), each r x n uint8."""
    rows = [str(s).upper() for s in strings]
    if not rows or any(len(s) != len(rows[0]) for s in rows):
        raise ValueError("give at least one Pauli string, all of the same length")
    bad = set("".join(rows)) - set("IXYZ")
    if bad:
        raise ValueError(f"a Pauli string holds only I, X, Y and Z (got {sorted(bad)})")
    A = np.array([list(s) for s in rows]).reshape(len(rows), len(rows[0]))
    return ((A == "X") | (A == "Y")).astype(np.uint8), ((A == "Z") | (A == "Y")).astype(np.uint8)


def five_qubit_code() -> Tuple[np.ndarray, np.ndarray]:
    """The [[5,1,3]] code: the four cyclic shifts XZZXI, IXZZX, XIXZZ, ZXIXZ.  -> (Sx, Sz), each 4 x 5."""
    return paulis_to_symplectic(["XZZXI"[-k:] + "XZZXI"[:-k] if k else "XZZXI" for k in range(4)])


def clifford_deform(Hx, Hz, perms) -> Tuple[sp.csc_matrix, sp.csc_matrix]:
    """A CSS code (Hx, Hz) with a single-qubit Clifford on every qubit: perms[j] in 0 .. 5 indexes PAULI_PERMUTATIONS, the
    images of X, Y, Z on qubit j.  Rows of Hx first (an X-check takes the image of X), then rows of Hz (a Z-check takes the
    image of Z).  -> (Sx, Sz), sparse uint8 patterns of rx + rz rows; commutation is preserved."""
    X, Z = sp.csc_matrix(_dense_bits(Hx)), sp.csc_matrix(_dense_bits(Hz))
    if X.shape[1] != Z.shape[1]:
        raise AssertionError("Hx and Hz must have the same number of columns")
    n = X.shape[1]
    perms = np.asarray(perms, dtype=np.int64).reshape(-1)
    if perms.shape != (n,) or ((perms < 0) | (perms > 5)).any():
        raise ValueError(f"one permutation index in 0 .. 5 per qubit: expected {n} entries")
    img_x = np.array([PAULI_PERMUTATIONS[k][0] for k in perms])
    img_z = np.array([PAULI_PERMUTATIONS[k][2] for k in perms])
    zero_x, zero_z = sp.csc_matrix(X.shape, dtype=np.uint8), sp.csc_matrix(Z.shape, dtype=np.uint8)

    def part(letters):   # the columns of (Hx; Hz) whose image has that part
        in_x = sp.diags(np.isin(img_x, letters).astype(np.uint8))
        in_z = sp.diags(np.isin(img_z, letters).astype(np.uint8))
        M = sp.csc_matrix(sp.vstack([X @ in_x if n else zero_x, Z @ in_z if n else zero_z])).astype(np.uint8)
        M.eliminate_zeros()
        M.sort_indices()
        return M

    return part(["X", "Y"]), part(["Z", "Y"])


def xzzx_surface_code(d: int) -> Tuple[sp.csc_matrix, sp.csc_matrix]:
    """The XZZX surface code of distance d: the hypergraph product of two (d - 1) x d repetition checks with X and Z
    exchanged (permutation ZYX) on the second block of qubits.  n = d^2 + (d - 1)^2, 2 d (d - 1) stabilizers of weight 3
    and 4, every one a product of X and Z (no Y).  -> (Sx, Sz)."""
    d = int(d)
    if d < 2:
        raise ValueError("d must be >= 2")
    rep = np.zeros((d - 1, d), dtype=np.uint8)
    rep[np.arange(d - 1), np.arange(d - 1)] = 1
    rep[np.arange(d - 1), np.arange(1, d)] = 1
    Hx, Hz = hypergraph_product(rep, rep)
    perms = np.zeros(Hx.shape[1], dtype=np.int64)
    perms[d * d:] = 5
    return clifford_deform(Hx, Hz, perms)


def symplectic_product(Ax, Az, Bx, Bz) -> np.ndarray:
    """[a][b] = 1 where Pauli a of (Ax | Az) anticommutes with Pauli b of (Bx | Bz)."""
    Ax, Az, Bx, Bz = (_dense_bits(M) for M in (Ax, Az, Bx, Bz))
    return _gf2_matmul(Ax, Bz.T) ^ _gf2_matmul(Az, Bx.T)


def stabilizer_logicals(Sx, Sz) -> Tuple[np.ndarray, np.ndarray]:
    """Logical operators of the stabilizer code (Sx, Sz): -> (LSx, LSz), each 2k x n uint8, k = n - rank[Sx | Sz].  The
    rows commute with every stabilizer, are independent modulo the stabilizers, and are paired: row a anticommutes with
    row k + a and with no other row.  Host GF(2) elimination (the centralizer is the kernel of [Sz | Sx]) and symplectic
    Gram-Schmidt, for create time."""
    X, Z = _dense_bits(Sx), _dense_bits(Sz)
    if X.shape != Z.shape:
        raise AssertionError("Sx and Sz must have the same shape")
    if symplectic_product(X, Z, X, Z).any():
        raise AssertionError("Sx * Sz' + Sz * Sx' != 0 over GF(2): the stabilizers do not commute")
    n = X.shape[1]
    S = np.concatenate([X, Z], axis=1)
    S = S[_first_independent_rows(S)]
    K = _gf2_kernel(np.concatenate([Z, X], axis=1))          # (x | z) with Sz x + Sx z = 0: the centralizer
    both = np.concatenate([S, K], axis=0)
    keep = [i - S.shape[0] for i in _first_independent_rows(both) if i >= S.shape[0]]
    L = [K[i].copy() for i in keep]                           # a basis of the centralizer modulo the stabilizers
    k2 = len(L)
    if k2 != 2 * (n - S.shape[0]):
        raise AssertionError("the centralizer modulo the stabilizers has the wrong dimension")

    def anti(u, v):
        return int((u[:n] & v[n:]).sum() + (u[n:] & v[:n]).sum()) & 1

    firsts, seconds = [], []
    while L:
        v = L.pop(0)
        hit = next((i for i, w in enumerate(L) if anti(v, w)), None)
        if hit is None:
            raise AssertionError("the form on the logical space is degenerate")
        w = L.pop(hit)
        L = [u ^ (v if anti(u, w) else 0) ^ (w if anti(u, v) else 0) for u in L]
        firsts.append(v)
        seconds.append(w)
    out = np.array(firsts + seconds, dtype=np.uint8).reshape(k2, 2 * n)
    return np.ascontiguousarray(out[:, :n]), np.ascontiguousarray(out[:, n:])
