"""Batched numpy model of BP with guided decimation as include/qldpc_hip.h specifies it (qldpc_decim_decode_batch): the tests pin the GPU kernel to it.

A round is one leg of Relay-BP with gamma = 0 and bias in place of the prior; the leg is restated here (relay_model.relay_decode is one function with
its own leg bookkeeping) with the same operations in the same order: the check pass of min-sum with the compressed state (strict first minimum, sign
bits, alpha * min), s = 0.0 + the sum of R in ascending check order, V = s + bias.  Between rounds the unfixed columns are ordered by (|V| descending
with NaN as 0, column ascending) and the first min(per_round, unfixed) are frozen.  Shots of a round run in lock step.
"""
import numpy as np

from relay_model import _clip_nan


class Tables:
    """padded row and column views of a CSR matrix (edge k of row i = CSR edge indptr[i] + k; a column's edges in ascending row order)"""

    def __init__(self, indptr, indices, n):
        indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
        self.m, self.n, self.nnz = indptr.size - 1, int(n), indices.size
        deg = np.diff(indptr)
        self.rdeg = int(deg.max()) if self.m else 0
        self.kk = np.arange(self.rdeg)
        self.rvalid = self.kk[None, :] < deg[:, None]
        self.redge = np.where(self.rvalid, indptr[:-1, None] + self.kk[None, :], 0)
        self.rcol = indices[self.redge]
        order = np.argsort(indices, kind="stable")                 # CSR is row-major: a stable sort keeps ascending rows per column
        cdeg_of = np.bincount(indices, minlength=self.n)
        cptr = np.concatenate([[0], np.cumsum(cdeg_of)])
        self.cdeg = int(cdeg_of.max()) if self.n else 0
        dd = np.arange(self.cdeg)
        self.cvalid = dd[None, :] < cdeg_of[:, None]
        self.cedge = np.where(self.cvalid, order[np.minimum(cptr[:-1, None] + dd[None, :], max(indices.size - 1, 0))], 0)


def run_round(tab, synd, V, bias, alpha, clip_llr, T):
    """One round on the shots of V [B, n] (changed in place) -> (conv bool[B], iterations int[B])."""
    B = V.shape[0]
    conv = np.zeros(B, bool)
    itc = np.full(B, T, np.int64)
    idx = np.arange(B)                                             # the shots still iterating
    Rprev = np.zeros((B, tab.nnz))
    for it in range(T + 1):
        Vc = V[idx][:, tab.rcol]                                   # [b, m, rdeg]
        with np.errstate(invalid="ignore"):
            x = Vc if it == 0 else _clip_nan(Vc - Rprev[idx][:, tab.redge], clip_llr)
        csyn = synd[idx]
        par = csyn ^ (np.logical_and(Vc < 0.0, tab.rvalid[None]).sum(axis=2) & 1).astype(bool)
        if it >= 1:
            ok = ~par.any(axis=1)
            conv[idx[ok]] = True
            itc[idx[ok]] = it
            idx, x, csyn = idx[~ok], x[~ok], csyn[~ok]
        if it == T or idx.size == 0:
            break
        neg = ~(x >= 0.0) & tab.rvalid[None]
        sp = csyn ^ (neg.sum(axis=2) & 1).astype(bool)
        a = np.abs(x)
        b = idx.size
        min1, min2, arg = np.full((b, tab.m), np.inf), np.full((b, tab.m), np.inf), np.full((b, tab.m), 127)
        for k in range(tab.rdeg):
            ak, v = a[:, :, k], tab.rvalid[None, :, k]
            lt1 = v & (ak < min1)
            lt2 = v & ~lt1 & (ak < min2)
            min2 = np.where(lt1, min1, np.where(lt2, ak, min2))
            min1 = np.where(lt1, ak, min1)
            arg = np.where(lt1, k, arg)
        m1a, m2a = alpha * min1, alpha * min2
        mag = np.where(tab.kk[None, None, :] == arg[:, :, None], m2a[:, :, None], m1a[:, :, None])
        Rrow = np.where(sp[:, :, None] != neg, -mag, mag)
        Rnew = np.zeros((b, tab.nnz))
        Rnew[:, tab.redge[tab.rvalid]] = Rrow[:, tab.rvalid]
        s = np.zeros((b, tab.n))
        for d in range(tab.cdeg):
            s = s + np.where(tab.cvalid[None, :, d], Rnew[:, tab.cedge[:, d]], 0.0)
        with np.errstate(invalid="ignore"):
            V[idx] = s + bias[idx]
        Rprev[idx] = Rnew
    return conv, itc


def select(v, fixed, per_round):
    """The columns one decimation freezes: unfixed, by |v| descending (NaN as 0), then column ascending -> int array in that order."""
    free = np.flatnonzero(~fixed)
    a = np.abs(v[free])
    a = np.where(np.isnan(a), 0.0, a)
    order = np.lexsort((free, -a))                                 # last key first: -a ascending = a descending, ties by column
    return free[order[:per_round]]


def decim_decode(indptr, indices, n, syndromes, prior, alpha, clip_llr, t_round, max_rounds, per_round, fix_llr, trace=None):
    """-> (err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B], rounds int32[B], fixed int32[B]).
    trace: a list that receives (shot, round, columns frozen after that round in selection order, V of the shot before they were frozen)."""
    tab = Tables(indptr, indices, n)
    synd = (np.asarray(syndromes, np.int8).reshape(-1, tab.m) & 1).astype(bool)
    prior = np.asarray(prior, np.float64)
    B = synd.shape[0]
    V = np.tile(prior, (B, 1))
    bias = np.tile(prior, (B, 1))
    fixed = np.zeros((B, n), bool)
    conv = np.zeros(B, np.uint8)
    iters, rounds = np.zeros(B, np.int32), np.zeros(B, np.int32)
    live = np.arange(B)
    for r in range(max_rounds + 1):
        if live.size == 0:
            break
        Vl = V[live]
        c, itc = run_round(tab, synd[live], Vl, bias[live], alpha, clip_llr, t_round)
        V[live] = Vl
        iters[live] += itc.astype(np.int32)
        rounds[live] = r + 1
        conv[live[c]] = 1
        go = ~c & (r < max_rounds) & ~fixed[live].all(axis=1)
        live = live[go]
        for b in live:
            cols = select(V[b], fixed[b], per_round)
            before = V[b].copy()
            val = np.where(V[b, cols] < 0.0, -fix_llr, fix_llr)
            bias[b, cols] = val
            V[b, cols] = val
            fixed[b, cols] = True
            if trace is not None:
                trace.append((int(b), r, cols.copy(), before))
    return (V < 0.0).astype(np.int8), V, conv, iters, rounds, fixed.sum(axis=1).astype(np.int32)
