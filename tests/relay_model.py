"""Batched numpy model of Relay-BP as include/qldpc_hip.h specifies it (qldpc_relay_decode_batch): the tests pin the GPU kernel to it.

Every floating-point operation is the kernel's, one IEEE rounding each in the same order: the check pass of min-sum with the compressed
state (strict first minimum, sign bits, alpha * min), the variable pass s = 0.0 + sum of R in ascending check order, then
V = s + ((1 - gamma) * prior + gamma * V), where a V that is not finite enters the memory term as 0.0.  Shots run in lock step; each one has its own leg and iteration counters.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable uint arrays -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(k0) & _MASK, np.uint64(k1) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _MASK, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return [x.astype(np.uint32) for x in c]


def gamma_draws(shots, n, leg, seed, tag):
    """u16 draws w[B, n] of leg `leg` >= 1 for the global shot indices `shots`."""
    shots = np.asarray(shots, dtype=np.uint64).reshape(-1, 1)
    blk = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    dom = 0x52000000 | (int(tag) << 20) | int(leg)
    out = philox4x32_10(shots & _MASK, shots >> np.uint64(32), blk, dom, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    w = np.stack(out, axis=2).reshape(shots.shape[0], -1)[:, :n]
    return (w >> np.uint32(16)).astype(np.uint16)


def gammas(shots, n, leg, seed, tag, gamma_min, gamma_max):
    w = gamma_draws(shots, n, leg, seed, tag).astype(np.float64)
    return gamma_min + (gamma_max - gamma_min) * (w * (1.0 / 65536.0))


def weights(prior):
    """q_j = floor(clamp(prior_j * 2^20, +-2^40) + 0.5) as int64."""
    x = np.clip(np.asarray(prior, np.float64) * 1048576.0, -1099511627776.0, 1099511627776.0)
    return np.floor(x + 0.5).astype(np.int64)


def _clip_nan(x, clip):
    return np.where(np.isnan(x), 0.0, np.clip(x, -clip, clip))


def relay_decode(indptr, indices, n, syndromes, prior, seed, shot_begin=0, tag=0, alpha=1.0, clip_llr=20.0, gamma0=0.125, gamma_min=-0.24,
                 gamma_max=0.66, t0=80, tr=60, max_legs=300, stop_after=5):
    """-> (err int8[B, n], conv uint8[B], legs int32[B], iters int32[B], solutions int32[B])."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    m = indptr.size - 1
    synd = (np.asarray(syndromes, np.int8).reshape(-1, m) & 1).astype(bool)
    prior = np.asarray(prior, np.float64)
    B = synd.shape[0]
    deg = np.diff(indptr)
    rdeg = int(deg.max()) if m else 0
    # padded row view: edge k of row i = CSR edge indptr[i] + k
    kk = np.arange(rdeg)
    rvalid = kk[None, :] < deg[:, None]
    redge = np.where(rvalid, indptr[:-1, None] + kk[None, :], 0)
    rcol = indices[redge]
    # column view: the column's edges in ascending row order
    order = np.argsort(indices, kind="stable")                 # CSR is row-major, so a stable sort keeps ascending rows per column
    cdeg_of = np.bincount(indices, minlength=n)
    cptr = np.concatenate([[0], np.cumsum(cdeg_of)])
    cdeg = int(cdeg_of.max()) if n else 0
    dd = np.arange(cdeg)
    cvalid = dd[None, :] < cdeg_of[:, None]
    cedge = np.where(cvalid, order[np.minimum(cptr[:-1, None] + dd[None, :], max(indices.size - 1, 0))], 0)
    q = weights(prior)
    shots = shot_begin + np.arange(B, dtype=np.int64)

    V = np.tile(prior, (B, 1))
    Rprev = np.zeros((B, indices.size))
    leg = np.zeros(B, np.int64)
    it = np.zeros(B, np.int64)
    T = np.full(B, t0, np.int64)
    gam = np.full((B, n), float(gamma0))
    best = np.full(B, np.iinfo(np.int64).max, np.int64)
    nsol = np.zeros(B, np.int32)
    iters = np.zeros(B, np.int32)
    legs = np.zeros(B, np.int32)
    err = np.zeros((B, n), np.int8)
    done = np.zeros(B, bool)
    csyn = synd[:, :]
    while not done.all():
        act = ~done
        Vc = V[:, rcol]                                                         # [B, m, rdeg]
        first = (it == 0)[:, None, None]
        with np.errstate(invalid="ignore"):
            x = np.where(first, Vc, _clip_nan(Vc - Rprev[:, redge], clip_llr))
        par = csyn ^ (np.logical_and(Vc < 0.0, rvalid[None]).sum(axis=2) & 1).astype(bool)
        neg = ~(x >= 0.0) & rvalid[None]
        sp = csyn ^ (neg.sum(axis=2) & 1).astype(bool)
        a = np.abs(x)
        min1 = np.full((B, m), np.inf)
        min2 = np.full((B, m), np.inf)
        arg = np.full((B, m), 127)
        for k in range(rdeg):
            ak = a[:, :, k]
            v = rvalid[None, :, k]
            lt1 = v & (ak < min1)
            lt2 = v & ~lt1 & (ak < min2)
            min2 = np.where(lt1, min1, np.where(lt2, ak, min2))
            min1 = np.where(lt1, ak, min1)
            arg = np.where(lt1, k, arg)
        m1a, m2a = alpha * min1, alpha * min2
        mag = np.where(kk[None, None, :] == arg[:, :, None], m2a[:, :, None], m1a[:, :, None])
        Rrow = np.where(sp[:, :, None] != neg, -mag, mag)                       # R of edge k, as the next passes rebuild it
        Rnew = np.zeros_like(Rprev)
        Rnew[:, redge[rvalid]] = Rrow[:, rvalid]
        unsat = par.any(axis=1)
        conv = act & (it >= 1) & ~unsat
        legend = act & (conv | (it == T))
        cont = act & ~legend
        if cont.any():
            s = np.zeros((B, n))
            for d in range(cdeg):
                s = s + np.where(cvalid[None, :, d], Rnew[:, cedge[:, d]], 0.0)
            with np.errstate(invalid="ignore"):
                bias = (1.0 - gam) * prior[None, :] + gam * np.where(np.isfinite(V), V, 0.0)   # a non-finite marginal carries no memory
                Vn = s + bias
            V = np.where(cont[:, None], Vn, V)
            Rprev = np.where(cont[:, None], Rnew, Rprev)
            it = np.where(cont, it + 1, it)
        for b in np.flatnonzero(legend):
            iters[b] += it[b] if conv[b] else T[b]
            legs[b] = leg[b] + 1
            hard = V[b] < 0.0
            if conv[b]:
                nsol[b] += 1
                w = int(q[hard].sum())
                if w < best[b]:
                    best[b] = w
                    err[b] = hard
            if nsol[b] >= stop_after or leg[b] == max_legs:
                done[b] = True
                if nsol[b] == 0:
                    err[b] = hard
            else:
                leg[b] += 1
                it[b] = 0
                T[b] = tr
                gam[b] = gammas([shots[b]], n, leg[b], seed, tag, gamma_min, gamma_max)[0]
    return err, (nsol > 0).astype(np.uint8), legs, iters, nsol
