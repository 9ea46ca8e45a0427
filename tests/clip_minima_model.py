"""numpy models of the check update with the clip of Q = V - R taken two ways (tests only):

  edge    clip every edge, then signs, min1 / min2 (with multiplicity), the position of the first minimum: the reference's order
          (oracle/qldpc_oracle.c orc_minsum_decode, kernels.py:282-345);
  minima  signs, min1 / min2 and the selector on the UNCLIPPED values, then min(min1, clip) and min(min2, clip): what the clean undamped
          kernel of minsum_regular.hip computes (selector |t| == min1; "first" is the stored-first-minimum selector of the workgroup kernels' state).

`check_messages` is one check update on arrays of rows; `MinSumModel` is the whole decoder on a batch of syndromes with either form, and counts the
check updates that had at least one edge changed by the clip."""
import numpy as np


def clip_edges(t, clip):
    """q = 0 if NaN, else clamped to [-clip, clip] with the reference's comparisons (a value inside the range keeps its bits, -0.0 included)"""
    t = np.asarray(t, np.float64)
    q = np.where(t != t, 0.0, t)
    q = np.where(q > clip, clip, q)
    return np.where(q < -clip, -clip, q)


def _messages(q, mask, synd, alpha, min_clip, selector):
    """q [..., D] (unclipped when min_clip is not None), mask [..., D] edge exists, synd [...] in {0, 1} -> message words f64 [..., D]"""
    mag = np.where(mask, np.abs(q), np.inf)
    neg = mask & ~(q >= 0)                                       # `val >= 0` counts -0.0 (and nothing else below zero) as positive
    srt = np.sort(mag, axis=-1)
    min1 = srt[..., 0]
    min2 = srt[..., 1] if q.shape[-1] > 1 else np.full(min1.shape, np.inf)
    if selector == "first":
        first = np.argmin(mag, axis=-1)                          # the first strict minimum
        sel = np.arange(q.shape[-1]) == first[..., None]
    else:
        sel = mag == min1[..., None]                             # every position that attains the minimum
    if min_clip is not None:
        deg = mask.sum(axis=-1)
        min1 = np.minimum(min1, min_clip)
        min2 = np.where(deg > 1, np.minimum(min2, min_clip), min2)   # a degree-1 row has no second magnitude: +inf stays
    row_neg = (np.asarray(synd).astype(bool) ^ (neg.sum(axis=-1) % 2 == 1))
    sign = np.where(row_neg[..., None] ^ neg, -1.0, 1.0)         # sign of the row without the edge itself
    with np.errstate(invalid="ignore"):
        return (alpha * sign) * np.where(sel, min2[..., None], min1[..., None])


def check_messages(t, clip, alpha, synd, form, selector="equal", mask=None):
    """One check update from the unclipped t = V[col] - R_prev of each row -> message words."""
    t = np.asarray(t, np.float64)
    mask = np.ones(t.shape, bool) if mask is None else mask
    if form == "edge":
        return _messages(clip_edges(t, clip), mask, synd, alpha, None, "first")
    tt = np.where(t != t, 0.0, t)
    return _messages(tt, mask, synd, alpha, clip, selector)


def words(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


class MinSumModel:
    """Flooding min-sum of orc_minsum_decode on a batch, damping 1, dynamical alpha (1 - 2^-(it+1)), for any Tanner graph in CSR form."""

    def __init__(self, indptr, indices, n):
        indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
        self.m, self.n = len(indptr) - 1, int(n)
        deg = np.diff(indptr)
        self.D = int(deg.max())
        self.deg = deg
        self.cols = np.zeros((self.m, self.D), np.int64)
        self.mask = np.arange(self.D)[None, :] < deg[:, None]
        rows = np.repeat(np.arange(self.m), deg)
        pos = np.arange(len(indices)) - indptr[rows]
        self.cols[rows, pos] = indices
        # column side: the edges of a column in ascending check order (the order the reference's scatter-add meets them)
        flat = rows * self.D + pos
        order = np.lexsort((rows, indices))
        cdeg = np.bincount(indices, minlength=self.n)
        self.V = int(cdeg.max())
        cptr = np.concatenate([[0], np.cumsum(cdeg)])
        self.cedge = np.zeros((self.n, self.V), np.int64)
        self.cmask = np.arange(self.V)[None, :] < cdeg[:, None]
        self.cedge[indices[order], np.arange(len(indices)) - cptr[indices[order]]] = flat[order]

    def decode(self, synd, prior, max_iter, clip, form="edge", selector="equal", count_rows=None, count_at_least=1):
        """-> dict(hard int8 [B, n], llr f64 [B, n], iters int32 [B], conv uint8 [B], updates, clipped_updates).

        updates: the check updates that read clipped values (iterations >= 1 of shots still running, rows with an edge; count_rows restricts them
        to a boolean row mask); clipped_updates: those with at least `count_at_least` edges whose value the clip changed."""
        synd = np.asarray(synd).reshape(-1, self.m).astype(np.int64)
        prior = np.asarray(prior, np.float64)
        B = synd.shape[0]
        hard = np.zeros((B, self.n), np.int8)
        llr = np.zeros((B, self.n), np.float64)
        iters = np.full(B, max_iter - 1, np.int32)
        conv = np.zeros(B, np.uint8)
        live = np.arange(B)
        Q = np.broadcast_to(prior[self.cols], (B, self.m, self.D)).copy()       # unclipped inputs of the next check update
        rows_counted = (self.deg > 0) if count_rows is None else (np.asarray(count_rows, bool) & (self.deg > 0))
        updates = clipped = 0
        first = True
        with np.errstate(invalid="ignore", over="ignore"):
            for it in range(max_iter):
                alpha = 1.0 - 2.0 ** -(it + 1)
                s = synd[live]
                if first:
                    R = _messages(Q, self.mask, s, alpha, None, "first")                           # iteration 0 reads priors: no clip
                else:
                    changed = (self.mask & (np.abs(Q) > clip)).sum(axis=-1)[:, rows_counted]
                    updates += changed.size
                    clipped += int((changed >= count_at_least).sum())
                    R = check_messages(Q, clip, alpha, s, form, selector, self.mask)
                first = False
                Rf = np.where(self.mask, R, 0.0).reshape(len(live), -1)
                tot = np.zeros((len(live), self.n))
                for d in range(self.V):
                    tot = tot + np.where(self.cmask[:, d], Rf[:, self.cedge[:, d]], 0.0)
                values = tot + prior
                cand = (values < 0).astype(np.int64)
                ok = ((np.where(self.mask, cand[:, self.cols], 0).sum(axis=-1) & 1) == s).all(axis=1)
                hard[live], llr[live] = cand, values
                iters[live[ok]], conv[live[ok]] = it, 1
                Q = values[:, self.cols] - R
                live, Q = live[~ok], Q[~ok]
                if live.size == 0:
                    break
        return dict(hard=hard, llr=llr, iters=iters, conv=conv, updates=updates, clipped_updates=clipped)
