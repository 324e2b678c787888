"""Host mirror of Julia's ``BitMatrix`` memory layout (one bit per element).

A ``BitMatrix`` of ``rows x cols`` keeps element (r, c), zero-based, as bit ``k = c * rows + r`` of one flat bit
string: word ``k >> 6`` of ``chunks`` (``UInt64``), bit ``k & 63``, least significant bit first; columns are not padded
and the bits behind the last element stay zero.  That is what the reference's test and doctest hand ``batchdecode!`` as
``errors`` (test/test_bp_decoder.jl:26, belief_propagation.jl:217), and what ``ldpc_bp_decode_batch_bits`` reads and
writes in place (include/ldpc_mi355x.h).  Pure numpy.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


class BitMatrix:
    __slots__ = ("rows", "cols", "chunks")

    def __init__(self, rows: int, cols: int, chunks: np.ndarray = None):
        rows, cols = int(rows), int(cols)
        if rows < 0 or cols < 0:
            raise ValueError("negative dimension")
        nwords = (rows * cols + 63) >> 6
        if chunks is None:
            chunks = np.zeros(nwords, dtype=np.uint64)
        if not (isinstance(chunks, np.ndarray) and chunks.dtype == np.uint64 and chunks.ndim == 1
                and chunks.size == nwords and chunks.flags.c_contiguous):
            raise ValueError(f"chunks must be a contiguous uint64 vector of length {nwords}")
        self.rows, self.cols, self.chunks = rows, cols, chunks

    # -- the reference's matrix vocabulary ------------------------------------
    @property
    def shape(self) -> Tuple[int, int]:
        return (self.rows, self.cols)

    ndim = 2

    def __len__(self) -> int:
        return self.rows

    @classmethod
    def zeros(cls, rows: int, cols: int) -> "BitMatrix":
        return cls(rows, cols)

    @classmethod
    def from_dense(cls, X) -> "BitMatrix":
        """Pack a ``rows x cols`` array; an element is a set bit when it is non-zero."""
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("from_dense takes a matrix")
        out = cls(X.shape[0], X.shape[1])
        flat = (X != 0).ravel(order="F")                       # k = c * rows + r
        packed = np.packbits(flat, bitorder="little")          # bit k & 7 of byte k >> 3
        out.chunks.view(np.uint8)[:packed.size] = packed       # (little-endian words; the rest stays zero)
        return out

    def to_dense(self, dtype=np.uint8) -> np.ndarray:
        nbits = self.rows * self.cols
        flat = np.unpackbits(self.chunks.view(np.uint8), count=nbits, bitorder="little")
        return flat.reshape((self.rows, self.cols), order="F").astype(dtype, copy=False)

    def columns(self, lo: int, hi: int) -> Tuple[np.ndarray, int]:
        """``(chunks, bit0)`` of the columns [lo, hi): the whole word vector and the bit at which column `lo` starts --
        the pair the bits entries take as (words, bit0) with batch = hi - lo."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.cols:
            raise IndexError(f"columns [{lo}, {hi}) outside 0..{self.cols}")
        return self.chunks, lo * self.rows

    def column(self, c: int) -> np.ndarray:
        """Column c as a dense uint8 vector."""
        if not 0 <= c < self.cols:
            raise IndexError(c)
        k = np.arange(c * self.rows, (c + 1) * self.rows, dtype=np.int64)
        return ((self.chunks[k >> 6] >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)

    def trailing_bits_zero(self) -> bool:
        nbits = self.rows * self.cols
        return nbits % 64 == 0 or int(self.chunks[-1]) >> (nbits % 64) == 0

    def __eq__(self, other):
        return (isinstance(other, BitMatrix) and self.shape == other.shape
                and np.array_equal(self.chunks, other.chunks))

    __hash__ = None

    def __repr__(self) -> str:
        return f"BitMatrix({self.rows} x {self.cols})"
