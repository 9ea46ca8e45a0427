"""numpy model of the compare-free check update of the clean undamped kernel in csrc/minsum_regular.hip (tests only), word for word:

  signs       from the high words: spw = (syndrome bit << 31) ^ hi(t_0) ^ .. ^ hi(t_{D-1}); edge k takes bit 31 of spw ^ hi(t_k);
  magnitudes  leave-one-out minima from a suffix chain s_k = min(|t_k|, s_{k+1}) and a prefix chain p_k = min(|t_k|, p_{k-1}):
              mag_0 = s_1, mag_{D-1} = p_{D-2}, mag_k = min(p_{k-1}, s_{k+1});
  clip        in the two chain seeds only: p_0 = min(|t_0|, cmin), s_{D-1} = min(|t_{D-1}|, cmin), cmin = clip, or +inf at iteration 0;
  word        (alpha * mag_k) with bit 63 replaced by the sign bit (v_bfi_b32 on the high word).

No comparison, no sort and no selector appears below.  The inputs are the UNCLIPPED t = V[col] - R_prev of rows of equal degree; the identity needs
what the kernel's header states: no t is -0.0 or NaN, clip > 0.  `LooModel` is tests/clip_minima_model.py's decoder with this check update and with
the hard decisions and their parity taken from the posteriors' high words."""
import numpy as np

import clip_minima_model as CM

SIGN = np.uint32(0x80000000)


def hi_words(x):
    return (CM.words(x) >> np.uint64(32)).astype(np.uint32)


def loo_messages(t, clip, alpha, synd):
    """t f64 [..., D] unclipped, clip > 0 or None (iteration 0: no clip), synd [...] in {0, 1} -> message words f64 [..., D]"""
    t = np.ascontiguousarray(t, np.float64)
    D = t.shape[-1]
    assert D >= 3
    cmin = np.inf if clip is None else np.float64(clip)
    hi = hi_words(t)
    spw = np.asarray(synd).astype(np.uint32) << np.uint32(31)
    for k in range(D):
        spw = spw ^ hi[..., k]
    a = np.abs(t)
    suf = [None] * D
    suf[D - 1] = np.minimum(a[..., D - 1], cmin)
    for k in range(D - 2, 0, -1):
        suf[k] = np.minimum(a[..., k], suf[k + 1])
    out = np.empty(t.shape, np.uint64)
    pre = None
    for k in range(D):
        mag = suf[1] if k == 0 else pre if k == D - 1 else np.minimum(pre, suf[k + 1])
        sgn = spw ^ hi[..., k]
        if k < D - 1:
            pre = np.minimum(a[..., 0], cmin) if k == 0 else np.minimum(a[..., k], pre)
        prod = CM.words(alpha * mag)
        word_hi = ((prod >> np.uint64(32)).astype(np.uint32) & ~SIGN) | (sgn & SIGN)
        out[..., k] = (word_hi.astype(np.uint64) << np.uint64(32)) | (prod & np.uint64(0xFFFFFFFF))
    return out.view(np.float64)


class LooModel(CM.MinSumModel):
    """MinSumModel.decode with the update above, for regular graphs (every row of degree D)."""

    def decode(self, synd, prior, max_iter, clip):
        """-> dict(hard int8 [B, n], llr f64 [B, n], iters int32 [B], conv uint8 [B])"""
        assert self.mask.all(), "regular graphs only"
        synd = np.asarray(synd).reshape(-1, self.m).astype(np.int64)
        prior = np.asarray(prior, np.float64)
        B = synd.shape[0]
        hard = np.zeros((B, self.n), np.int8)
        llr = np.zeros((B, self.n), np.float64)
        iters = np.full(B, max_iter - 1, np.int32)
        conv = np.zeros(B, np.uint8)
        live = np.arange(B)
        Q = np.broadcast_to(prior[self.cols], (B, self.m, self.D)).copy()
        for it in range(max_iter):
            alpha = 1.0 - 2.0 ** -(it + 1)
            s = synd[live]
            R = loo_messages(Q, None if it == 0 else clip, alpha, s)
            Rf = R.reshape(len(live), -1)
            tot = np.zeros((len(live), self.n))
            for d in range(self.V):
                tot = tot + np.where(self.cmask[:, d], Rf[:, self.cedge[:, d]], 0.0)
            values = tot + prior
            vhi = hi_words(values)
            cand = (vhi >> np.uint32(31)).astype(np.int64)                       # hard decision = sign bit of the posterior's high word
            par = np.bitwise_xor.reduce(vhi[:, self.cols], axis=-1) >> np.uint32(31)   # parity of a row = sign bit of the XOR of its high words
            ok = (par.astype(np.int64) == s).all(axis=1)
            hard[live], llr[live] = cand, values
            iters[live[ok]], conv[live[ok]] = it, 1
            Q = values[:, self.cols] - R
            live, Q = live[~ok], Q[~ok]
            if live.size == 0:
                break
        return dict(hard=hard, llr=llr, iters=iters, conv=conv)
