"""Numpy model of the single-precision flooding min-sum decoder (include/qldpc_hip.h, qldpc_minsum32_decoder_create), the statement the library is
pinned to bit for bit.  Batched over the shots, vectorised over the rows (check pass) and the columns (variable pass); every value is np.float32 and
every arithmetic step is one numpy f32 operation: am = alpha * mag, R = +-am, s = s + R in ascending check order, V = s + prior32, Q = V - R.  numpy
promotes silently (an f32 array times a Python float of an f64 array is f64), so the dtypes are asserted where they could slip.  Plain module (no
pytest hooks)."""
import numpy as np

F32 = np.float32


def alpha_table32(max_iter, alpha_mode, alpha):
    """alpha_k of qldpc_minsum_decode_batch in f64 ('dynamical' 1 - 2^-(k+1); 'const' alpha; 'seq' alpha[min(k, len - 1)]), then rounded to f32"""
    if alpha_mode == "dynamical":
        tab = np.array([1.0 - 2.0 ** (-(k + 1)) for k in range(max_iter)], np.float64)
    elif alpha_mode == "const":
        tab = np.full(max_iter, float(alpha), np.float64)
    else:
        seq = np.asarray(alpha, np.float64)
        tab = np.array([seq[min(k, len(seq) - 1)] for k in range(max_iter)], np.float64)
    with np.errstate(over="ignore"):
        return tab.astype(F32)


class Minsum32Model:
    def __init__(self, indptr, indices, n, prior):
        self.indptr, self.indices, self.n = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), int(n)
        self.m = len(indptr) - 1
        with np.errstate(over="ignore"):
            self.prior32 = np.asarray(prior, np.float64).astype(F32)            # round to nearest even; +-inf and NaN pass through
        deg = np.diff(self.indptr)
        self.rows = np.flatnonzero(deg > 0)                                      # rows without entries are skipped
        D = int(deg.max()) if len(deg) and deg.max() > 0 else 1
        self.eid = np.zeros((len(self.rows), D), np.int64)
        self.rmask = np.zeros((len(self.rows), D), bool)
        for r, i in enumerate(self.rows):
            k = int(deg[i])
            self.eid[r, :k] = np.arange(self.indptr[i], self.indptr[i + 1])
            self.rmask[r, :k] = True
        self.row_of_edge = np.repeat(np.arange(self.m), deg)
        # per column: its edges in ascending check order (CSR edge ids ascend with the row)
        order = np.argsort(self.indices, kind="stable")
        cdeg = np.bincount(self.indices, minlength=self.n)
        Cd = int(cdeg.max()) if len(self.indices) else 1
        self.ceid = np.zeros((self.n, Cd), np.int64)
        self.cmask = np.zeros((self.n, Cd), bool)
        start = np.concatenate([[0], np.cumsum(cdeg)])
        for j in range(self.n):
            k = int(cdeg[j])
            self.ceid[j, :k] = order[start[j]:start[j] + k]
            self.cmask[j, :k] = True

    def syndrome_of(self, e):
        """H e over GF(2) for e [B, n] -> [B, m]"""
        out = np.zeros((e.shape[0], self.m), np.int64)
        if len(self.indices):
            np.add.at(out, (slice(None), self.row_of_edge), e[:, self.indices].astype(np.int64))
        return (out & 1).astype(np.int8)

    def decode(self, syndromes, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0):
        """-> (err int8[B, n], conv uint8[B], llr f64[B, n] (the f32 V widened), final_iter int32[B])"""
        synd = (np.asarray(syndromes, np.int8).reshape(-1, self.m) & 1)
        B = synd.shape[0]
        alphas = alpha_table32(max_iter, alpha_mode, alpha)
        clip = F32(clip_llr)
        assert np.isfinite(clip) and clip > 0, "clip_llr must be finite and > 0 as an f32"
        inf = F32(np.inf)
        Q = np.tile(self.prior32[self.indices], (B, 1))                          # iteration 0: Q = prior32, unclipped
        V = np.tile(self.prior32, (B, 1))
        conv, iters = np.zeros(B, np.uint8), np.full(B, max_iter - 1, np.int32)
        act = np.arange(B)
        D = self.eid.shape[1]
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(max_iter):
                if act.size == 0:
                    break
                a = alphas[k]
                Qa = Q[act]
                # ---- check pass
                Qp = Qa[:, self.eid]                                             # [b, rows, D]
                neg = self.rmask & ~(Qp >= 0)                                    # the sign is + for Q >= 0
                ab = np.abs(Qp)
                ab = np.where(self.rmask & ~np.isnan(ab), ab, inf)               # a NaN never passes the strict < of the scan: like +inf
                assert ab.dtype == F32
                pos = np.argmin(ab, axis=2)                                      # the first position of the minimum
                min1 = np.take_along_axis(ab, pos[..., None], axis=2)[..., 0]
                rest = ab.copy()
                np.put_along_axis(rest, pos[..., None], inf, axis=2)
                min2 = rest.min(axis=2)                                          # degree 1: +inf
                sp = (synd[act][:, self.rows].astype(bool)) ^ (np.count_nonzero(neg, axis=2) & 1).astype(bool)
                mag = np.where(np.arange(D)[None, None, :] == pos[..., None], min2[..., None], min1[..., None])
                am = a * mag                                                     # ONE f32 multiply
                assert am.dtype == F32 and mag.dtype == F32 and a.dtype == F32
                Rp = np.where(sp[..., None] ^ neg, -am, am)
                R = np.zeros_like(Qa)
                R[:, self.eid[self.rmask]] = Rp[:, self.rmask]
                # ---- variable pass: s = 0.0f + R in ascending check order, one add each
                s = np.zeros((len(act), self.n), F32)
                for d in range(self.ceid.shape[1]):
                    s = np.where(self.cmask[:, d], s + R[:, self.ceid[:, d]], s)
                Va = s + self.prior32
                Qn = Va[:, self.indices] - R
                assert s.dtype == F32 and Va.dtype == F32 and Qn.dtype == F32 and R.dtype == F32
                Qn = np.where(np.isnan(Qn), F32(0.0), Qn)
                Qn = np.where(Qn > clip, clip, np.where(Qn < -clip, -clip, Qn))
                assert Qn.dtype == F32
                Q[act], V[act] = Qn, Va
                ok = (self.syndrome_of((Va < 0).astype(np.int8)) == synd[act]).all(axis=1)
                conv[act[ok]] = 1
                iters[act[ok]] = k
                act = act[~ok]
        assert V.dtype == F32 and Q.dtype == F32
        return (V < 0).astype(np.int8), conv, V.astype(np.float64), iters
