"""Seeded matrices for the literal GF(2) Gauss-Jordan routine (eliminate_packed, csrc/gf2.hip) behind qldpc_gf2_eliminate and qldpc_gf2_eliminate_packed: the
edges of its accepted domain, each on the smallest matrix that shows it.  tests/test_elim_domain_cpu.py checks with the oracle and a plain numpy elimination
that every case holds what it is named for; tests/test_elim_domain_gpu.py runs them.  Plain module (no pytest hooks); deterministic from osd_shapes.SEED.

A case is B matrices A [B, m, n] (bytes) with right-hand sides b [B, m]; what it expects per shot -- rank, row swaps, the last pivot's column -- is written in
TABLE by hand.  `packed3` is the one case given in packed form only: three row words for n = 70, random bits set beyond column 70 (the entry point asks
for nwords * 64 >= n, no more): those bits never pivot but are XOR-ed like any other."""
from types import SimpleNamespace

import numpy as np

import osd_shapes as OS
from osdw_shapes import ELIM_MAX, elim_lds_bytes, nwords_of          # noqa: F401 (ELIM_MAX: for the modules that use this table)

LDS_TEXT = "matrix too large for the LDS scratch"
ERR_UNSUPPORTED = -4


def _rng(name, *what):
    return OS._rng("elim:" + name, *what)


def block_of(m):
    return 1024 if m >= 512 else 256           # the launch of both entry points


def _random(name, m, n, p=0.3, zero_rows=()):
    A = (_rng(name).random((1, m, n)) < p).astype(np.uint8)
    A[0, list(zero_rows)] = 0
    return A


def _dep(name, m, n):
    """random sparse rows; row 3 = row 0 + row 1, rows 5 and 6 equal, row 2 empty"""
    A = _random(name, m, n, 0.15)
    A[0, 3] = A[0, 0] ^ A[0, 1]
    A[0, 6] = A[0, 5]
    A[0, 2] = 0
    return A


def _tall8(name, m):
    """m rows over 8 columns, the first 40 rows empty and ones only in every 7th row after: every pivot is found far below `row` and swapped up"""
    A = _random(name, m, 8, 0.5, range(40))
    A[0, np.arange(m) % 7 != 0] = 0
    return A


def _ones_at(m, n, where):
    A = np.zeros((1, m, n), np.uint8)
    for r, c in where:
        A[0, r, c] = 1
    return A


def _antidiag(n):
    return np.eye(n, dtype=np.uint8)[::-1][None].copy()


def _shift(n):
    return np.roll(np.eye(n, dtype=np.uint8), 1, axis=1)[None].copy()          # row i has its one in column i + 1: the pivot of every column is the LAST row


def _zero_first(n):
    rng = _rng("zero_first")
    U = np.triu((rng.random((n, n)) < 0.4).astype(np.uint8), 1) | np.eye(n, dtype=np.uint8)
    return np.concatenate([np.zeros((1, n), np.uint8), U])[None].copy()


def _last_col(n):
    A = np.zeros((1, 3, n), np.uint8)
    A[0, 0, [0, 5, n - 1]] = 1
    A[0, 1, [1, 5]] = 1
    A[0, 2, n - 1] = 1
    return A


def _ranks(name, m, n, ranks):
    rng = _rng(name)
    out = []
    for r in ranks:
        if r == min(m, n):
            out.append((np.eye(m, n, dtype=np.uint8) + np.triu((rng.random((m, n)) < 0.3), 1)) % 2)
        else:
            out.append(((rng.random((m, r)) < 0.5).astype(np.int64) @ (rng.random((r, n)) < 0.5).astype(np.int64)) % 2)
    return np.array(out, np.uint8)


# name -> (builder, expectations per shot, note)
TABLE = {
    "e511x40": (lambda: _dep("e511x40", 511, 40), dict(rank=[40], swaps=[36], last=[39]), "the last matrix on 256 threads"),
    "e512x40": (lambda: _dep("e512x40", 512, 40), dict(rank=[40], swaps=[36], last=[39]), "the first on 1024 threads"),
    "lds_13097": (lambda: _tall8("lds", 13097), dict(rank=[8], swaps=[8], last=[7]), "65533 bytes of scratch: the last launch within 64 KiB"),
    "lds_13098": (lambda: _tall8("lds", 13098), dict(rank=[8], swaps=[8], last=[7]), "65538 bytes: the first launch above 64 KiB"),
    "lds_30710": (lambda: _tall8("lds", 30710), dict(rank=[8], swaps=[8], last=[7]), "153598 bytes: the last accepted"),
    "lds_30711": (lambda: _tall8("lds", 30711), dict(refused=True), "153603 bytes: refused"),
    "e1x1": (lambda: np.ones((1, 1, 1), np.uint8), dict(rank=[1], swaps=[0], last=[0]), "one entry"),
    "e1x64": (lambda: _ones_at(1, 64, [(0, 9), (0, 30), (0, 63)]), dict(rank=[1], swaps=[0], last=[9]), "one row, one full word"),
    "e64x1": (lambda: _ones_at(64, 1, [(63, 0)]), dict(rank=[1], swaps=[1], last=[0]), "one column, its one in the last row"),
    "antidiag65": (lambda: _antidiag(65), dict(rank=[65], swaps=[32], last=[64]), "anti-diagonal: the pivot of column c is row 64 - c until the middle"),
    "shift65": (lambda: _shift(65), dict(rank=[65], swaps=[64], last=[64]), "a cyclic shift: a swap at every step but the last"),
    "zero_first": (lambda: _zero_first(20), dict(rank=[20], swaps=[20], last=[19]), "an empty row sits at `row` at every step while the pivot is found below it"),
    "last_col64": (lambda: _last_col(64), dict(rank=[3], swaps=[0], last=[63]), "the last pivot's only one in column n - 1 = 63"),
    "last_col65": (lambda: _last_col(65), dict(rank=[3], swaps=[0], last=[64]), "the same in the first bit of the second word"),
    "ones70": (lambda: np.ones((1, 70, 70), np.uint8), dict(rank=[1], swaps=[0], last=[0]), "all ones: one pivot clears 69 rows of two words"),
    "batch5": (lambda: _ranks("batch5", 40, 70, (40, 0, 1, 13, 27)), dict(rank=[40, 0, 1, 13, 27], swaps=[0, 0, 0, 9, 11], last=[39, -1, 1, 13, 29]),
               "five matrices in one launch: rank min(m, n), 0, 1 and two in between"),
}
PACKED3 = "packed3"
_CASES = {}


def case(name):
    if name not in _CASES:
        build, expect, note = TABLE[name]
        A = np.ascontiguousarray(build(), np.uint8)
        B, m, n = A.shape
        b = (_rng(name, 9).random((B, m)) < 0.5).astype(np.uint8)
        _CASES[name] = SimpleNamespace(name=name, A=A, b=b, B=B, m=m, n=n, nwords=nwords_of(n), expect=expect, note=note, refused=expect.get("refused", False),
                                       lds=elim_lds_bytes(m, nwords_of(n)))
    return _CASES[name]


def packed3():
    """-> (P uint64 [1, 30, 3], b uint8 [1, 30], n = 70): random bits in all 192 positions of a row"""
    rng = _rng(PACKED3)
    P = rng.integers(0, 1 << 63, (1, 30, 3), dtype=np.uint64) ^ (rng.integers(0, 2, (1, 30, 3), dtype=np.uint64) << np.uint64(63))
    P[0, 4] = P[0, 1] ^ P[0, 2]
    return P, (rng.random((1, 30)) < 0.5).astype(np.uint8), 70


def plain_elimination(A, b):
    """column by column, the first row at or below `row` -> (A, b, pivot_rows, pivot_cols, swaps)"""
    A, b = A.copy(), b.copy()
    m, n = A.shape
    row, pr, pc, swaps = 0, [], [], 0
    for col in range(n):
        if row >= m:
            break
        nz = np.flatnonzero(A[row:, col])
        if nz.size == 0:
            continue
        p = row + int(nz[0])
        if p != row:
            A[[row, p]], b[[row, p]] = A[[p, row]], b[[p, row]]
            swaps += 1
        rest = np.flatnonzero(A[:, col])
        rest = rest[rest != row]
        A[rest] ^= A[row]
        b[rest] ^= b[row]
        pr.append(row)
        pc.append(col)
        row += 1
    return A, b, pr, pc, swaps

