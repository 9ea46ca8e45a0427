"""Models and case table for csrc/passes.hip: the two single check passes, the sum-product driver and the estimator statistics.

The models are the reference's own statements (bp_core, kernels.py:171-193; performBeliefPropagationFast, dense.py:75-96) on CSR, once
in mpmath at 50 digits (`*_mp`, the yardstick) and once line by line in numpy f64 (`*_f64`, what the reference's arithmetic gives).
Their inputs are exact doubles.  test_passes_cpu.py ties the f64 models to the oracle and to the reference's recorded outputs and
measures how far f64 strays from the 50-digit values; test_passes_gpu.py holds the kernels to the 50-digit values.

Tolerances
  single pass   pass_tolerance(deg, pc, R) = u * ((2 deg + 4) * 2|pc| / (1 - pc^2) + 2|R|) + 1e-290, u = 2^-53: deg - 1 roundings of the
                product, those of the factors, the division and the sign (<= 2 deg + 4 in all) reach R = 2 atanh(pc) through
                dR/dpc = 2 / (1 - pc^2); 2|R| u is the atanh and its doubling.  The floor covers rows whose product underflows (22 or
                more clamped factors): there f64 and the exact value are both below 1e-300.
  driver        per case d_ref = max |f64 model - mp model| over every iteration's values, tol = 100 * max(d_ref, 16 u max|value|).
                A case is stable when both models agree on every decision (hence on convergence and iteration) and the smallest
                |value| of the mp model exceeds 1e4 * tol; only stable cases are compared in value and decision.

The `flaw` arguments exist for test_passes_cpu.py's sensitivity check alone: each names one deliberate mistake, and the comparison the
GPU tests make (pass_ratio, driver_failures, column_sums) has to reject it on at least one case of the table.
"""
import functools
import os

import mpmath
import numpy as np

U = 2.0 ** -53
CLIP = 0.9999999          # CLIP_VAL of dense.py:84
TINY = 1e-15              # the tanh clamp of kernels.py:181-182
DPS = 50
BATCHES = (1, 3, 257, 1000)
MAX_ITERS = (1, 2, 10)
PASS_FLAWS = ("clamp_1e-14", "clamp_sign_gt", "clip_0.999999", "no_syndrome_sign", "no_divide")
DRIVER_FLAWS = ("prior_first", "stale_Q", "done_overwritten", "iter_is_max_iter")
DISCRETE = np.array([0.0, -0.0, 1e-17, -1e-17, -1e-300, 40.0, -40.0, 700.0, np.inf, -np.inf])
CLAMPED = DISCRETE[:5]    # the members whose tanh is clamped


# ---- single check pass ----------------------------------------------------------------------------------------------------
def bp_pass_mp(indptr, indices, Q, ssign, clip_val=CLIP):
    """bp_core at 50 digits on one shot -> (R, pc): per edge the message and the clipped product, lists of mpf."""
    nnz = len(indices)
    R, PC = [mpmath.mpf(0)] * nnz, [mpmath.mpf(0)] * nnz
    with mpmath.workdps(DPS):
        tiny, clip = mpmath.mpf(TINY), mpmath.mpf(float(clip_val))
        for i in range(len(indptr) - 1):
            rs, re = int(indptr[i]), int(indptr[i + 1])
            th = []
            for pos in range(rs, re):
                q = Q[pos] if isinstance(Q[pos], mpmath.mpf) else mpmath.mpf(float(Q[pos]))      # the mp driver hands its Q over unrounded
                t = mpmath.tanh(q * 0.5)
                if abs(t) < tiny:
                    t = tiny if t >= 0 else -tiny                     # mpf has no signed zero: -0.0 >= 0, as in IEEE
                th.append(t)
            row_prod = mpmath.mpf(1)
            for t in th:
                row_prod *= t
            ss = mpmath.mpf(float(ssign[i]))
            for pos, t in zip(range(rs, re), th):
                pc = (row_prod / t) * ss
                pc = min(max(pc, -clip), clip)
                PC[pos] = pc
                R[pos] = 2 * mpmath.atanh(pc)
    return R, PC


def bp_pass_f64(indptr, indices, Q, ssign, clip_val=CLIP, flaw=None):
    """bp_core line by line in numpy f64 on one shot -> R f64[nnz]."""
    tiny = 1e-14 if flaw == "clamp_1e-14" else TINY
    clip = np.float64(0.999999 if flaw == "clip_0.999999" else clip_val)
    Q = np.asarray(Q, np.float64)
    R = np.zeros(len(indices))
    with np.errstate(all="ignore"):
        for i in range(len(indptr) - 1):
            rs, re = int(indptr[i]), int(indptr[i + 1])
            th = np.tanh(Q[rs:re] * 0.5)
            pos_sign = (th > 0) if flaw == "clamp_sign_gt" else (th >= 0)
            th = np.where(np.abs(th) < tiny, np.where(pos_sign, tiny, -tiny), th)
            row_prod = np.float64(1.0)
            for t in th:
                row_prod = row_prod * t
            ss = np.float64(1.0 if flaw == "no_syndrome_sign" else ssign[i])
            for k in range(re - rs):
                pc = (row_prod if flaw == "no_divide" else row_prod / th[k]) * ss
                pc = np.clip(pc, -clip, clip)
                R[rs + k] = 2.0 * np.arctanh(pc)
    return R


def pass_tolerance(deg, pc, R):
    pc, R = np.abs(np.asarray(pc, np.float64)), np.abs(np.asarray(R, np.float64))
    return U * ((2.0 * deg + 4.0) * 2.0 * pc / (1.0 - pc * pc) + 2.0 * R) + 1e-290


def edge_degrees(indptr):
    return np.repeat(np.diff(indptr), np.diff(indptr)).astype(np.float64)


def column_edges(indptr, indices, n):
    """per column the CSR positions of its edges, in ascending row order"""
    cols = [[] for _ in range(n)]
    for pos, j in enumerate(indices):
        cols[int(j)].append(pos)
    return cols


def column_sums(indptr, indices, n, R, prior=None):
    """((0 + R[e1]) + R[e2]) + ... in ascending row order, then + prior: np.sum(R, axis=0) and dense.py:88-89 in f64, R f64[B, nnz]"""
    R = np.atleast_2d(np.asarray(R, np.float64))
    out = np.zeros((R.shape[0], n))
    with np.errstate(all="ignore"):
        for j, edges in enumerate(column_edges(indptr, indices, n)):
            for pos in edges:
                out[:, j] = out[:, j] + R[:, pos]
        if prior is not None:
            out = out + np.asarray(prior, np.float64)
    return out


# ---- driver ------------------------------------------------------------------------------------------------------------------
def _syndrome_of(indptr, indices, hard):
    return np.array([int(np.bitwise_xor.reduce(hard[indices[indptr[i]:indptr[i + 1]]], initial=0)) for i in range(len(indptr) - 1)], np.int8)


def bp_decode_mp(indptr, indices, n, syndrome, prior, max_iter):
    """performBeliefPropagationFast at 50 digits -> dict(err int8[n], conv, iter, values: one list of n mpf per iteration run)."""
    indices = np.asarray(indices)
    syndrome = np.asarray(syndrome, np.int8).reshape(-1)
    cols = column_edges(indptr, indices, n)
    with mpmath.workdps(DPS):
        pri = [mpmath.mpf(float(x)) for x in prior]
        ssign = [1.0 - 2.0 * int(s) for s in syndrome]
        Q = [pri[int(j)] for j in indices]
        values, conv, hard = [], False, np.zeros(n, np.int8)
        for it in range(max_iter):
            R, _ = bp_pass_mp(indptr, indices, Q, ssign)
            v = []
            for j in range(n):
                s = mpmath.mpf(0)
                for pos in cols[j]:
                    s += R[pos]
                v.append(s + pri[j])
            values.append(v)
            Q = [v[int(j)] - R[pos] for pos, j in enumerate(indices)]
            hard = np.array([1 if x < 0 else 0 for x in v], np.int8)
            if np.array_equal(_syndrome_of(indptr, indices, hard), syndrome):
                conv = True
                break
    return dict(err=hard, conv=conv, iter=it, values=values)


def bp_decode_f64(indptr, indices, n, syndrome, prior, max_iter, flaw=None):
    """performBeliefPropagationFast line by line in numpy f64 -> dict(err, conv, iter, values f64[iterations run, n])."""
    indices = np.asarray(indices)
    syndrome = np.asarray(syndrome, np.int8).reshape(-1)
    prior = np.asarray(prior, np.float64)
    ssign = 1.0 - 2.0 * syndrome.astype(np.float64)
    Q = prior[indices].copy() if len(indices) else np.zeros(0)
    values, conv, hard, first = [], False, np.zeros(n, np.int8), None
    pass_flaw = flaw if flaw in PASS_FLAWS else None
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            R = bp_pass_f64(indptr, indices, Q, ssign, CLIP, pass_flaw)
            if flaw == "prior_first":
                v = prior.copy()
                for j, edges in enumerate(column_edges(indptr, indices, n)):
                    for pos in edges:
                        v[j] = v[j] + R[pos]
            else:
                v = column_sums(indptr, indices, n, R, prior)[0]
            values.append(v)
            if not (flaw == "stale_Q" and it == 0):
                Q = v[indices] - R if len(indices) else Q
            hard = (v < 0).astype(np.int8)
            if np.array_equal(_syndrome_of(indptr, indices, hard), syndrome):
                conv = True
                if flaw == "done_overwritten":
                    first = it if first is None else first
                    continue
                break
    if flaw == "done_overwritten" and first is not None:
        return dict(err=hard, conv=True, iter=first, values=np.array(values))
    if flaw == "iter_is_max_iter" and not conv:
        it = max_iter
    return dict(err=hard, conv=conv, iter=it, values=np.array(values).reshape(-1, n))


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def _csr(rows, n):
    indptr = np.zeros(len(rows) + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.array([j for r in rows for j in sorted(r)], np.int32)
    return indptr, indices, int(n)


def _golden(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
    with np.load(path) as d:
        return {k: d[k] for k in d.files}


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> (indptr, indices, n).  'irregular': rows of degree 1, 0, 3, 2, column 5 without an edge; 'wide': rows of degree 56, 23
    and 4 (the product of 22 or more clamped factors underflows); 'norows': 0 x 4."""
    rng = np.random.default_rng(20261020)
    g = _golden("core_passes")
    out = {"core": (g["indptr"].astype(np.int32), g["indices"].astype(np.int32), int(g["shape"][1]))}
    # 12 x 24, every row of degree 4, every column of degree 2: a random pairing of the 48 edge stubs, redrawn until no row repeats a column
    while True:
        stubs = rng.permutation(np.repeat(np.arange(24), 2)).reshape(12, 4)
        if all(len(set(r)) == 4 for r in stubs):
            break
    out["random4"] = _csr([list(r) for r in stubs], 24)
    out["irregular"] = _csr([[2], [], [0, 2, 4], [1, 3], [0, 1, 3, 4]], 6)
    out["wide"] = _csr([list(range(56)), list(range(40, 63)), [0, 20, 41, 62], [1, 57]], 64)
    out["norows"] = _csr([], 4)
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    c = load_code("bb72")
    out["bb72"] = (np.asarray(c["Hx_indptr"], np.int32), np.asarray(c["Hx_indices"], np.int32), int(c["n"]))
    return out


def degree1_graph():
    """every row of degree 1: every min-sum check message is +-inf"""
    return _csr([[0], [2], [1]], 4)


FAMILIES = ("n3", "n30", "n1e-3", "discrete")


def draw(family, rng, shape, wide_cols=None):
    """one input family; on `wide_cols` (the edges of rows of degree >= 22) the discrete family draws clamped members only"""
    if family == "discrete":
        x = rng.choice(DISCRETE, size=shape)
        if wide_cols is not None and wide_cols.any():
            x[..., wide_cols] = rng.choice(CLAMPED, size=x[..., wide_cols].shape)
        return x
    return rng.normal(0.0, {"n3": 3.0, "n30": 30.0, "n1e-3": 1e-3}[family], shape)


def batch_rows(B, distinct):
    """row b of a batch of B is distinct row batch_rows(B, D)[b]: a fixed permutation of repeats, so neighbours differ"""
    return np.random.default_rng(1000 + B).permutation(np.arange(B) % distinct)


# ---- single-pass cases -------------------------------------------------------------------------------------------------------
PASS_DISTINCT = 8


@functools.lru_cache(maxsize=None)
def pass_cases():
    """One case per (graph, family): PASS_DISTINCT distinct shots with the mp model's message, clipped product, tolerance and column
    sums, all read-only.  A batch of B gathers these rows through batch_rows(B, PASS_DISTINCT)."""
    cases = []
    for gi, (gname, (indptr, indices, n)) in enumerate(graphs().items()):
        m, nnz = len(indptr) - 1, len(indices)
        deg = edge_degrees(indptr)
        wide = deg >= 22
        cols = column_edges(indptr, indices, n)
        for fi, fam in enumerate(FAMILIES):
            rng = np.random.default_rng([20261020, gi, fi])
            D = PASS_DISTINCT
            Q = draw(fam, rng, (D, nnz), wide)
            ssign = np.where(rng.random((D, m)) < 0.5, -1.0, 1.0)
            R, PC, S = np.zeros((D, nnz)), np.zeros((D, nnz)), np.zeros((D, n))
            Rmp = []
            for d in range(D):
                r, pc = bp_pass_mp(indptr, indices, Q[d], ssign[d])
                Rmp.append(r)
                R[d], PC[d] = [float(x) for x in r], [float(x) for x in pc]
                with mpmath.workdps(DPS):
                    S[d] = [float(mpmath.fsum(r[pos] for pos in cols[j])) for j in range(n)]
            tol = pass_tolerance(deg, PC, R).reshape(D, nnz)
            tol_sum = np.array([[tol[d, cols[j]].sum() if cols[j] else 0.0 for j in range(n)] for d in range(D)]).reshape(D, n)
            case = dict(name=f"{gname}-{fam}", graph=gname, family=fam, indptr=indptr, indices=indices, n=n, m=m, nnz=nnz, Q=Q, ssign=ssign,
                        R=R, pc=PC, tol=tol, Rsum=S, tol_sum=tol_sum, R_mp=Rmp)
            for a in (Q, ssign, R, PC, tol, S, tol_sum):
                a.setflags(write=False)
            cases.append(case)
    return cases


def pass_ratio(case, rows, R, Rsum=None):
    """largest |R - mp| / pass_tolerance over a batch whose row b is the case's distinct row rows[b] (and the same for R_sum against
    the sum of its edges' tolerances; a column without edges must hold 0).  inf where a value is not finite."""
    R = np.asarray(R, np.float64).reshape(len(rows), case["nnz"])
    worst = 0.0
    if R.size:
        if not np.isfinite(R).all():
            return np.inf
        worst = float(np.max(np.abs(R - case["R"][rows]) / case["tol"][rows]))
    if Rsum is not None and case["n"]:
        Rsum = np.asarray(Rsum, np.float64).reshape(len(rows), case["n"])
        if not np.isfinite(Rsum).all():
            return np.inf
        d, t = np.abs(Rsum - case["Rsum"][rows]), case["tol_sum"][rows]
        if (d[t == 0] != 0).any():
            return np.inf
        if (t > 0).any():
            worst = max(worst, float(np.max(d[t > 0] / t[t > 0])))
    return worst


# ---- driver cases ------------------------------------------------------------------------------------------------------------
DRIVER_FAMILIES = ("llr", "n3", "n30", "n1e-3")
DRIVER_DISTINCT = 8
BATCH_CASE = "random4-llr"          # the case the B = 257 / 1000 batches come from: 32 distinct syndromes
BATCH_DISTINCT = 32


def driver_prior(family, rng, n):
    """Priors matching the input families.  'llr' is a channel prior log((1 - q) / q), q in [0.02, 0.2]; 'n3' is N(0, 3) as drawn (both
    signs: the decoder rarely converges); 'n30' and 'n1e-3' are |N(0, sigma)| kept away from zero, so that shots converge at iteration 0
    and later and the posteriors keep a margin; 'discrete' (one graph only, it is unstable by construction: exact zeros) is the finite
    part of the discrete set."""
    if family == "llr":
        q = rng.uniform(0.02, 0.2, n)
        return np.log((1 - q) / q)
    if family == "n3":
        return rng.normal(0.0, 3.0, n)
    if family == "n30":
        return np.abs(rng.normal(0.0, 30.0, n)) + 2.0
    if family == "n1e-3":
        return np.abs(rng.normal(0.0, 1e-3, n)) + 2e-4
    return rng.choice(DISCRETE[:8], size=n)


def _syndromes(indptr, indices, n, m, count, rng, prior):
    """the zero syndrome seen through the prior's own signs (converges at iteration 0), single and double errors on top of it, and
    random syndromes (mostly not realisable: never converge), in that order"""
    base = (np.asarray(prior) < 0).astype(np.int8)
    out = []
    for k in range(count):
        e = base.copy()
        if k % 4 in (1, 2) and n:
            e[rng.choice(n, min(n, 1 + k % 3), replace=False)] ^= 1
        s = _syndrome_of(indptr, indices, e)
        if k % 4 == 3 and m:
            s = (rng.random(m) < 0.5).astype(np.int8)
        out.append(s)
    return np.array(out, np.int8).reshape(count, m)


@functools.lru_cache(maxsize=None)
def driver_cases():
    """One case per (graph, family, syndrome) at max_iter = 10, with both models' trajectories, d_ref, tol and the stable flag.  A run
    with max_iter = k < 10 is the prefix of the same trajectory (the driver keeps no state but Q), see expected()."""
    cases = []
    for gi, (gname, (indptr, indices, n)) in enumerate(graphs().items()):
        m = len(indptr) - 1
        fams = DRIVER_FAMILIES + (("discrete",) if gname == "irregular" else ())
        for fi, fam in enumerate(fams):
            rng = np.random.default_rng([20261021, gi, fi])
            prior = driver_prior(fam, rng, n)
            prior.setflags(write=False)
            count = BATCH_DISTINCT if f"{gname}-{fam}" == BATCH_CASE else DRIVER_DISTINCT
            if gname == "norows":
                count = 1
            synd = _syndromes(indptr, indices, n, m, count, rng, prior)
            for k in range(count):
                mp_ = bp_decode_mp(indptr, indices, n, synd[k], prior, 10)
                f = bp_decode_f64(indptr, indices, n, synd[k], prior, 10)
                V = np.array([[float(x) for x in v] for v in mp_["values"]]).reshape(-1, n)
                agree = f["values"].shape == V.shape and np.array_equal(f["values"] < 0, V < 0)
                both = min(len(V), len(f["values"]))
                d_ref = float(np.max(np.abs(f["values"][:both] - V[:both]))) if both and n else 0.0
                vmax = float(np.max(np.abs(V))) if V.size else 0.0
                tol = 100.0 * max(d_ref, 16 * U * vmax)
                vmin = float(np.min(np.abs(V))) if V.size else np.inf
                stable = bool(agree and np.isfinite(d_ref) and vmin > 1e4 * tol)
                V.setflags(write=False)
                cases.append(dict(name=f"{gname}-{fam}-{k}", group=f"{gname}-{fam}", graph=gname, family=fam, indptr=indptr, indices=indices, n=n,
                                  m=m, syndrome=synd[k], prior=prior, values=V, f64=f, conv=mp_["conv"], iter=mp_["iter"], d_ref=d_ref, tol=tol,
                                  margin=vmin, stable=stable))
    return cases


def expected(case, max_iter):
    """what the mp model returns for this case at max_iter <= 10 -> (err, conv, iter, values of the returned iteration)"""
    if case["conv"] and case["iter"] < max_iter:
        it, conv = case["iter"], True
    else:
        it, conv = max_iter - 1, False
    v = case["values"][it]
    return (v < 0).astype(np.int8), conv, it, v


def driver_failures(case, max_iter, err, conv, it, llr):
    """The comparison of one driver result with the mp model -> list of what is wrong (empty: accepted).  Every case must return finite
    values of the model's shape; a stable case must also give the model's decisions, flag and iteration and values within tol."""
    bad = []
    llr = np.asarray(llr, np.float64)
    if llr.shape != (case["n"],) or np.asarray(err).shape != (case["n"],):
        return ["shape"]
    if not np.isfinite(llr).all():
        bad.append("not finite")
    if not case["stable"]:
        return bad
    e, c, i, v = expected(case, max_iter)
    if not np.array_equal(np.asarray(err, np.int8), e):
        bad.append("decisions")
    if bool(conv) != c:
        bad.append("converged")
    if int(it) != i:
        bad.append(f"iteration {int(it)} != {i}")
    if case["n"] and not np.max(np.abs(llr - v)) <= case["tol"]:
        bad.append(f"values off by {np.max(np.abs(llr - v)) / case['tol']:.3g} tol")
    return bad


def driver_deviation(case, max_iter, llr):
    """|llr - model| in units of the case's tol (stable cases)"""
    v = expected(case, max_iter)[3]
    return float(np.max(np.abs(np.asarray(llr) - v)) / case["tol"]) if case["n"] and case["tol"] > 0 else 0.0
