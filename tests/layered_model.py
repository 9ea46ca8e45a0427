"""Numpy model of the layered-schedule min-sum decoder (include/qldpc_hip.h, qldpc_layered_decoder_create), the statement the library is pinned to
bit for bit.  Vectorised over the checks of a layer and over the shots: inside a layer no two checks share a column, so the gather / scatter below
touches every posterior once and no floating-point sum has an order to choose.  Every arithmetic step is one numpy f64 operation (no fused
multiply-add): R = (alpha * (sign_prod * sign)) * mag, V = Q + R.  Plain module (no pytest hooks)."""
import numpy as np


def greedy_layers(indptr, indices, n):
    """Rows in ascending index; a row gets the smallest layer >= 0 that no earlier row sharing a column with it holds (no entries: layer 0)."""
    m = len(indptr) - 1
    held = [set() for _ in range(n)]
    out = np.zeros(m, np.int32)
    for i in range(m):
        cols = [int(j) for j in indices[indptr[i]:indptr[i + 1]]]
        taken = set().union(*[held[j] for j in cols]) if cols else set()
        c = 0
        while c in taken:
            c += 1
        out[i] = c
        for j in cols:
            held[j].add(c)
    return out


def layers_valid(indptr, indices, n, row_layer):
    """no two rows of one layer share a column"""
    seen = set()
    for i in range(len(indptr) - 1):
        for j in indices[indptr[i]:indptr[i + 1]]:
            key = (int(row_layer[i]), int(j))
            if key in seen:
                return False
            seen.add(key)
    return True


def alpha_table(max_iter, alpha_mode, alpha):
    """alpha_k of qldpc_minsum_decode_batch: 'dynamical' 1 - 2^-(k+1); 'const' alpha; 'seq' alpha[min(k, len - 1)]"""
    if alpha_mode == "dynamical":
        return np.array([1.0 - 2.0 ** (-(k + 1)) for k in range(max_iter)])
    if alpha_mode == "const":
        return np.full(max_iter, float(alpha))
    seq = np.asarray(alpha, np.float64)
    return np.array([seq[min(k, len(seq) - 1)] for k in range(max_iter)])


class LayeredModel:
    def __init__(self, indptr, indices, n, prior, row_layer=None):
        self.indptr, self.indices, self.n = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), int(n)
        self.m = len(indptr) - 1
        self.prior = np.asarray(prior, np.float64)
        self.row_layer = greedy_layers(indptr, indices, n) if row_layer is None else np.asarray(row_layer)
        deg = np.diff(self.indptr)
        self.stages = []                                  # per layer that runs: rows, padded columns / edge ids [rows, maxdeg], mask
        for lay in np.unique(self.row_layer[deg > 0]):
            rows = np.flatnonzero((self.row_layer == lay) & (deg > 0))
            d = int(deg[rows].max())
            cols, eid, mask = np.zeros((len(rows), d), np.int64), np.zeros((len(rows), d), np.int64), np.zeros((len(rows), d), bool)
            for r, i in enumerate(rows):
                k = int(deg[i])
                cols[r, :k] = self.indices[self.indptr[i]:self.indptr[i + 1]]
                eid[r, :k] = np.arange(self.indptr[i], self.indptr[i + 1])
                mask[r, :k] = True
            self.stages.append((rows, cols, eid, mask))
        self.row_of_edge = np.repeat(np.arange(self.m), deg)

    def layer_sizes(self):
        return [len(st[0]) for st in self.stages]

    def syndrome_of(self, e):
        """H e over GF(2) for e [B, n] -> [B, m]"""
        out = np.zeros((e.shape[0], self.m), np.int64)
        if len(self.indices):
            np.add.at(out, (slice(None), self.row_of_edge), e[:, self.indices].astype(np.int64))
        return (out & 1).astype(np.int8)

    @staticmethod
    def two_minima(ab):
        """ab [B, rows, maxdeg], +inf beyond a row's degree -> (position of the minimum, the minimum, the minimum of the other positions).  A method
        of its own so that a test can put another rule in its place (a subclass) and see what its inputs can tell apart."""
        pos = np.argmin(ab, axis=2)                                               # the first position of the minimum
        min1 = np.take_along_axis(ab, pos[..., None], axis=2)[..., 0]
        rest = ab.copy()
        np.put_along_axis(rest, pos[..., None], np.inf, axis=2)
        return pos, min1, rest.min(axis=2)                                        # degree 1: +inf

    def decode(self, syndromes, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0):
        """-> (err int8[B, n], conv uint8[B], llr f64[B, n], final_iter int32[B])"""
        synd = (np.asarray(syndromes, np.int8).reshape(-1, self.m) & 1)
        B = synd.shape[0]
        alphas = alpha_table(max_iter, alpha_mode, alpha)
        V = np.tile(self.prior, (B, 1))
        R = np.zeros((B, len(self.indices)))
        ss = 1.0 - 2.0 * synd
        conv, iters = np.zeros(B, np.uint8), np.full(B, max_iter - 1, np.int32)
        act = np.arange(B)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(max_iter):
                if act.size == 0:
                    break
                a = alphas[k]
                Va, Ra = V[act], R[act]
                for rows, cols, eid, mask in self.stages:
                    Q = Va[:, cols] - Ra[:, eid]
                    Q = np.where(np.isnan(Q), 0.0, Q)
                    Q = np.where(Q > clip_llr, clip_llr, np.where(Q < -clip_llr, -clip_llr, Q))
                    sg = np.where(mask, np.where(Q >= 0, 1.0, -1.0), 1.0)
                    ab = np.where(mask, np.abs(Q), np.inf)
                    pos, min1, min2 = self.two_minima(ab)
                    sign_prod = ss[act][:, rows] * np.prod(sg, axis=2)
                    mag = np.where(np.arange(ab.shape[2])[None, None, :] == pos[..., None], min2[..., None], min1[..., None])
                    Rn = a * (sign_prod[..., None] * sg) * mag
                    Vn = Q + Rn
                    Va[:, cols[mask]] = Vn[:, mask]
                    Ra[:, eid[mask]] = Rn[:, mask]
                V[act], R[act] = Va, Ra
                ok = (self.syndrome_of((Va < 0).astype(np.int8)) == synd[act]).all(axis=1)
                conv[act[ok]] = 1
                iters[act[ok]] = k
                act = act[~ok]
        return (V < 0).astype(np.int8), conv, V, iters
