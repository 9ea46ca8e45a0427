"""Numpy model of the detector-error-model sampler as include/qldpc_hip.h specifies it (qldpc_circuit_plan_create_dem), built on the Philox of
tests/relay_model.py: the tests pin the GPU kernel to it bit for bit.  Also the tiny model the CPU and GPU tests share."""
import numpy as np

from relay_model import philox4x32_10

DOMAIN = 3


def thresholds(prob):
    """thr_l = floor(p_l * 2^32) as uint32 (0 <= p < 1; the product is exact in f64)."""
    prob = np.asarray(prob, np.float64)
    assert ((prob >= 0) & (prob < 1)).all()
    return np.floor(prob * 4294967296.0).astype(np.uint64).astype(np.uint32)


def fires(prob, seed, trial_begin, count):
    """bool[count, n_mech]: mechanism l of trial g = trial_begin + t fires iff word l & 3 of Philox(counter (lo g, hi g, l >> 2, 3), key seed) < thr_l."""
    prob = np.asarray(prob, np.float64)
    n = prob.size
    g = (np.uint64(trial_begin) + np.arange(count, dtype=np.uint64)).reshape(-1, 1)
    blk = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    o = philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), blk, DOMAIN, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    words = np.stack(o, axis=2).reshape(count, -1)[:, :n]
    return words < thresholds(prob).reshape(1, -1)


def sample(dem, seed, trial_begin, count):
    """[(syndromes int8[count, n_det], true int8[count, k]) per sector] of a qldpc_amd.simulation.dem.DetectorErrorModel."""
    f = fires(dem.prob, seed, trial_begin, count)
    out = []
    for S in dem.sectors:
        D = np.zeros((dem.n_mech, S.n_det), np.int64)          # mechanisms x detectors
        Lg = np.zeros((dem.n_mech, max(S.k, 1)), np.int64)
        for l in range(dem.n_mech):
            D[l, S.det_idx[S.det_ptr[l]:S.det_ptr[l + 1]].astype(np.int64)] = 1
            for r in range(S.k):
                Lg[l, r] = (int(S.logmask[l]) >> r) & 1
        fi = f.astype(np.int64)
        out.append((((fi @ D) & 1).astype(np.int8), ((fi @ Lg) & 1).astype(np.int8)[:, :S.k]))
    return out


TINY_NDET, TINY_K = (37, 5), (64, 3)


def tiny_dem(DetectorErrorModel, layer_rows=None):
    """Two sectors with 37 and 5 detectors (neither a multiple of 32, one below 32), k = (64, 3) (bit 63 in use), 37 mechanisms (a ragged Philox
    block), among them p = 0, thr = 1, p = 0.5, one empty in both sectors, one hitting both sectors, one with the highest detector and bit 63."""
    prob, cols = [], []
    special = {0: (0.0, ([0, 1], 1), ([0], 1)),                              # p = 0: never fires
               1: (2.0 ** -32, ([2], 2), ([], 0)),                           # thr = 1
               2: (0.5, ([0, 1, 3, 4], 0), ([], 0)),
               3: (0.3, ([], 0), ([], 0)),                                   # empty in both sectors
               4: (0.2, ([5, 36], 1 << 7), ([1, 4], 4)),                     # hits both sectors
               5: (0.15, ([36], 1 << 63), ([], 0)),                          # highest detector index, bit 63
               6: (0.1, ([], 1 << 62), ([], 0)),                             # an undetectable logical flip
               36: (0.25, ([35], 0), ([4], 2))}                              # the lone mechanism of the last Philox block
    for l in range(37):
        if l in special:
            p, c0, c1 = special[l]
        else:                                                                # every detector of both sectors is flipped by some mechanism
            p = (0.02, 0.05, 0.1)[l % 3]
            c0 = (sorted({l, (7 * l + 3) % 37} | ({6} if l == 7 else set())), (1 << (5 * l) % 64) if l % 2 else 0)
            t = l // 3
            c1 = (sorted({t % 5, (t + 2) % 5} if t % 2 else {t % 5}), l % 8) if l % 3 == 0 else ([], 0)
        prob.append(p)
        cols.append((c0, c1))
    dem = DetectorErrorModel.from_columns(prob, cols, TINY_NDET, TINY_K, layer_rows=layer_rows)
    # The decoder's view need not have the truth's columns: sector 0 decodes on the derived view plus six single-detector columns (p = 0.01, no logical),
    # which also makes its matrix wider than tall (37 x 40), as every decoding matrix here is.
    import scipy.sparse as sp
    v = dem.decoder_view(0)
    H = sp.csr_matrix((np.ones(v.indices.size, np.int8), v.indices, v.indptr), shape=v.shape)
    H = sp.hstack([H, sp.csr_matrix((np.ones(6, np.int8), (np.arange(6), np.arange(6))), shape=(v.shape[0], 6))]).tocsr()
    H.sort_indices()
    wide = type(v)(H.indptr.astype(np.int32), H.indices.astype(np.int32), H.shape, np.concatenate([v.prior, np.full(6, np.log(0.99 / 0.01))]),
                   np.concatenate([v.logmask, np.zeros(6, np.uint64)]))
    return DetectorErrorModel(dem.prob, [tuple(S) for S in dem.sectors], [wide, None])


# ---- the same sampler and the trial judge at sizes the dense products above cannot take (tests/dem_shapes.py) --------------------------------------
def sample_sparse(dem, seed, trial_begin, count):
    """`sample` without the count x n_mech x n_det products: the same fires(), then per sector the mechanisms' detector lists as one sparse
    n_mech x n_det matrix and the logical masks XOR-ed over every trial's firing mechanisms."""
    import scipy.sparse as sp
    f = fires(dem.prob, seed, trial_begin, count)
    F = sp.csr_matrix(f.astype(np.int32))
    out = []
    for S in dem.sectors:
        ptr = S.det_ptr.astype(np.int64)
        D = sp.csr_matrix((np.ones(ptr[-1], np.int32), S.det_idx.astype(np.int64), ptr), shape=(dem.n_mech, S.n_det))
        synd = (np.asarray((F @ D).todense()) & 1).astype(np.int8).reshape(count, S.n_det)
        acc = np.array([np.bitwise_xor.reduce(S.logmask[f[t]], initial=np.uint64(0)) for t in range(count)], np.uint64).reshape(count)
        out.append((synd, unpack_logicals(acc, S.k)))
    return out


def unpack_logicals(acc, k):
    """uint64[count] -> int8[count, k], bit r in column r"""
    acc = np.asarray(acc, np.uint64).reshape(-1, 1)
    return ((acc >> np.arange(k, dtype=np.uint64).reshape(1, -1)) & np.uint64(1)).astype(np.int8).reshape(acc.shape[0], k)


def pack_logicals(true):
    """int8[count, k] -> uint64[count]"""
    true = np.asarray(true)
    acc = np.zeros(true.shape[0], np.uint64)
    for r in range(true.shape[1]):
        acc |= (true[:, r].astype(np.uint64) & np.uint64(1)) << np.uint64(r)
    return acc


def predict(view, det):
    """uint64[count]: the XOR of the view's logical masks over the ones of every correction"""
    det = np.asarray(det)
    return np.array([np.bitwise_xor.reduce(view.logmask[(det[b] & 1) != 0], initial=np.uint64(0)) for b in range(det.shape[0])], np.uint64).reshape(det.shape[0])


def judge(view, syndromes, det, true):
    """What csrc/judge.h decides per trial, on the host: (logical error, unsatisfied = H @ det != s somewhere, zero syndrome), three bool[count].
    view: a DecoderView; syndromes int8[count, m]; det int8[count, n]; true int8[count, k]."""
    import scipy.sparse as sp
    m, n = view.shape
    syndromes, det = np.asarray(syndromes).reshape(-1, m), np.asarray(det).reshape(-1, n)
    H = sp.csr_matrix((np.ones(view.indices.size, np.int32), view.indices.astype(np.int64), view.indptr.astype(np.int64)), shape=(m, n))
    par = (np.asarray(H @ (det.T & 1).astype(np.int32)).reshape(m, -1).T & 1)
    s = syndromes & 1
    return predict(view, det) != pack_logicals(true), (par != s).any(axis=1), ~s.any(axis=1)


JUDGE_SPARSE_ROWS = 4096


def judge_is_dense(ms):
    """The form rule of circuit_run and events_predict_launch, restated: the row-wise (dense) judge runs as soon as one sector has more rows than the
    4096 parity bits a trial owns per sector in LDS (every graph carries its column lists, so nothing else decides)."""
    return any(m > JUDGE_SPARSE_ROWS for m in ms)
