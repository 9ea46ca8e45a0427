"""The logical error rate as a function of p from ONE sweep over the number of faults (subset sampling).  New here: the reference has no counterpart.

The circuit sampler draws each of its N fault locations independently with one probability p, so the number of faults of a trial is Binomial(N, p) and,
given that number, the faulty set is uniform.  The failure fraction f_w at exactly w faults therefore does not depend on p, and

    LER(p) = sum_w C(N, w) p^w (1 - p)^(N - w) f_w.

``run_weight_strata`` measures f_w with the plan's fixed-weight sampler (``_lib.CircuitPlan.use_fixed_weight``, the law in ``include/qldpc_hip.h``) for a
range of w on one plan, and ``WeightStrata.logical_error_rate(p)`` evaluates the sum for any p.  The trials go to the weights where failures are, and the
binomial mass of the weights that were not run bounds the truncation rigorously (``lower`` / ``upper``).

The decoder is held fixed across the sweep: ``prior_error_rate`` is the p the decoding matrices and the priors are built at, and f_w belongs to THAT
decoder configuration (matrices, priors, decoder, maxIter, ...).  ``logical_error_rate(p)`` is what that fixed decoder reaches at physical rate p; a decoder
whose priors follow p is another decoder, and another sweep.

``run_dem_weight_strata`` does the same for a ``DetectorErrorModel`` whose mechanisms all have one probability (a non-uniform model has no weight strata
of this kind: that needs conditional Bernoulli sampling and is out of scope).

A sweep runs on a single device.  Sharding it over several GPUs or ranks is out of scope.
"""
import math

import numpy as np

from .. import _lib
from . import dem as dem_mod, engine

T = _lib.TALLY
STRATUM_SHIFT = 40          # weight w uses the global trial range starting at w << 40: strata never share a Philox counter


def log_binomial_coefficient(n, w):
    """log C(n, w).  lgamma(n + 1) - lgamma(w + 1) - lgamma(n - w + 1) cancels three numbers of size n log n (an absolute error of 3e-11 at the
    17 280 locations of the [[144,12,12]] circuit), so the large factorials are never formed: with m = min(w, n - w),
    log C(n, w) = sum_{i < m} log(n - i) - lgamma(m + 1), the sum exactly rounded (math.fsum)."""
    m = min(w, n - w)
    return math.fsum(math.log(n - i) for i in range(m)) - math.lgamma(m + 1)


def log_binomial_pmf(n, w, p):
    """log of C(n, w) p^w (1 - p)^(n - w) (-inf where the mass is 0)."""
    if not 0 <= w <= n:
        return -math.inf
    if p <= 0.0:
        return 0.0 if w == 0 else -math.inf
    if p >= 1.0:
        return 0.0 if w == n else -math.inf
    return log_binomial_coefficient(n, w) + w * math.log(p) + (n - w) * math.log1p(-p)


def binomial_pmf(n, weights, p):
    """B_w(p) for every w of `weights` and every p of `p` -> f64[len(p), len(weights)]."""
    p = np.atleast_1d(np.asarray(p, np.float64)).ravel()
    n = int(n)
    logc = [log_binomial_coefficient(n, int(w)) for w in weights]
    out = np.zeros((p.size, len(logc)), np.float64)
    for a, q in enumerate(p.tolist()):
        if not 0.0 < q < 1.0:
            out[a] = [math.exp(log_binomial_pmf(n, int(w), q)) for w in weights]
            continue
        lp, lq = math.log(q), math.log1p(-q)
        out[a] = [math.exp(c + int(w) * lp + (n - int(w)) * lq) for c, w in zip(logc, weights)]
    return out


def weights_for(n_locs, p_range, coverage=1e-9):
    """The contiguous weight range (lo, hi), both inclusive, for physical rates p_lo .. p_hi: from the `coverage` quantile of Binomial(N, p_lo) to the
    1 - `coverage` quantile of Binomial(N, p_hi).  The binomial mass below lo at p_lo and above hi at p_hi is each <= coverage (and smaller for every
    p in between, where both tails lie further out)."""
    n = int(n_locs)
    p_lo, p_hi = float(p_range[0]), float(p_range[1])
    if not (0.0 < p_lo <= p_hi < 1.0):
        raise ValueError(f"p_range must be (p_lo, p_hi) with 0 < p_lo <= p_hi < 1, got {p_range!r}")
    if not 0.0 < coverage < 0.5:
        raise ValueError(f"coverage must be in (0, 0.5), got {coverage!r}")
    lo, acc = 0, 0.0                       # the largest lo with P(W < lo) <= coverage at p_lo
    for logb in _log_pmf_walk(n, p_lo):
        acc += math.exp(logb)
        if acc > coverage or lo == n:
            break
        lo += 1
    # The upper tail at p_hi.  The walk stops at `cut`, beyond the mode, where the pmf is 1e-30 of `coverage`; from there on the ratio
    # r_w = B_{w+1} / B_w < 1 only falls, so the mass above `cut` is at most B_cut r / (1 - r): the sum starts from that bound, never from less.
    mode, floor = int((n + 1) * p_hi), math.log(coverage) - 69.0
    logs = []
    for logb in _log_pmf_walk(n, p_hi):
        logs.append(logb)
        if len(logs) - 1 > mode and logb < floor:
            break
    cut = len(logs) - 1
    r = (n - cut) / (cut + 1.0) * (p_hi / (1.0 - p_hi))
    hi, acc = cut, (math.exp(logs[cut]) * r / (1.0 - r) if cut < n else 0.0)         # the smallest hi with P(W > hi) <= coverage at p_hi
    while hi > lo:
        acc += math.exp(logs[hi])
        if acc > coverage:
            break
        hi -= 1
    return lo, hi


def _log_pmf_walk(n, p):
    """log B_w(p) for w = 0, 1, .. n, one step each: log B_0 = n log(1 - p) and log B_{w+1} = log B_w + log((n - w) / (w + 1)) + log(p / (1 - p)), the sum
    compensated (Neumaier), so that a walk of 1e5 steps still agrees with log_binomial_pmf to a few ulp.  It costs what it walks: picking a weight
    range is O(hi), not O(N hi)."""
    odds = math.log(p) - math.log1p(-p)
    s, comp = n * math.log1p(-p), 0.0
    yield s
    for w in range(n):
        x = math.log((n - w) / (w + 1.0)) + odds
        t = s + x
        comp += (s - t) + x if abs(s) >= abs(x) else (x - t) + s
        s = t
        yield s + comp


def _check_sweep_args(weights, p_range, coverage, trials_per_weight, target_failures, max_trials_per_weight, batch):
    """The argument rules of a sweep that need no plan, before any device call -> (weights as a list of ints or None, cap of trials per weight)."""
    if weights is None and p_range is None:
        raise ValueError("give weights=... (an iterable of fault counts) or p_range=(p_lo, p_hi)")
    if weights is not None and p_range is not None:
        raise ValueError("give weights=... or p_range=..., not both")
    if weights is not None:
        weights = [_lib.check_fixed_weight(w) for w in weights]
        if not weights:
            raise ValueError("weights is empty")
        if min(weights) < 0 or max(weights) > _lib.FIXED_WEIGHT_MAX:
            raise ValueError(f"weights must lie in 0..{_lib.FIXED_WEIGHT_MAX} (the sampler's limit), got {min(weights)}..{max(weights)}")
        if len(set(weights)) != len(weights):
            raise ValueError("weights holds a fault count twice")
    else:
        weights_for(1, p_range, coverage)                  # (the rules of p_range and coverage)
    if int(trials_per_weight) < 1:
        raise ValueError("trials_per_weight must be >= 1")
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    if target_failures is not None and int(target_failures) < 1:
        raise ValueError("target_failures must be >= 1 (or None)")
    if max_trials_per_weight is not None and target_failures is None:
        raise ValueError("max_trials_per_weight is for target_failures=...")
    cap = int(trials_per_weight) if target_failures is None else int(max_trials_per_weight if max_trials_per_weight is not None else trials_per_weight)
    if cap < 1 or cap >= 1 << STRATUM_SHIFT:
        raise ValueError(f"a stratum holds 1..2^{STRATUM_SHIFT} - 1 trials")
    return weights, cap


def _resolve_weights(n_locs, weights, p_range, coverage):
    """The weights of a sweep once N is known -> int64[]: the explicit ones, or the contiguous range of p_range, cut at the sampler's limit."""
    n_locs = int(n_locs)
    if n_locs > _lib.FIXED_WEIGHT_MAX_LOCS:
        raise ValueError(f"{n_locs} fault locations are above the fixed-weight sampler's limit of {_lib.FIXED_WEIGHT_MAX_LOCS}")
    top = min(n_locs, _lib.FIXED_WEIGHT_MAX)
    if weights is None:
        lo, hi = weights_for(n_locs, p_range, coverage)
        if hi > top:
            raise ValueError(f"p_range={p_range!r} needs weights up to {hi}, above the sampler's limit of {top} faults per trial")
        weights = range(lo, hi + 1)
    elif max(weights) > top:
        raise ValueError(f"weight {max(weights)} is above the {n_locs} fault locations")
    return np.array(list(weights), np.int64)


class WeightStrata:
    """What a sweep measured: ``n_locs`` (N) and, per sampled weight, ``trials``, ``failures`` (either sector), ``failures_z`` / ``failures_x`` and
    ``bp_converged`` (int64[len(weights), 2]: trials whose BP stage converged in sector Z / X, from the tally)."""

    FIELDS = ("weights", "trials", "failures", "failures_z", "failures_x", "bp_converged")

    def __init__(self, n_locs, weights, trials, failures, failures_z, failures_x, bp_converged):
        self.n_locs = int(n_locs)
        self.weights, self.trials, self.failures, self.failures_z, self.failures_x = (np.asarray(a, np.int64).ravel() for a in
                                                                                       (weights, trials, failures, failures_z, failures_x))
        self.bp_converged = np.asarray(bp_converged, np.int64).reshape(self.weights.size, 2)
        if not (self.weights.size == self.trials.size == self.failures.size == self.failures_z.size == self.failures_x.size):
            raise ValueError("one entry per weight is needed in every array")
        if np.unique(self.weights).size != self.weights.size or (self.weights.size and (self.weights.min() < 0 or self.weights.max() > self.n_locs)):
            raise ValueError("weights must be distinct and inside 0..n_locs")

    def save(self, path):
        np.savez(path, n_locs=np.int64(self.n_locs), **{k: getattr(self, k) for k in self.FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as d:
            return cls(int(d["n_locs"]), *(d[k] for k in cls.FIELDS))

    def logical_error_rate(self, p):
        """LER(p) for a scalar or an array p -> a dict of f64 arrays of p's shape:
          estimate   sum over the sampled w of B_w(p) k_w / n_w, B_w the Binomial(N, p) pmf (a weight with no trial counts as not sampled)
          std_error  sqrt(sum B_w^2 v_w / n_w), v_w = q (1 - q), q = (k_w + 1) / (n_w + 2): a stratum without failures does not claim zero variance
          covered    sum of B_w over the sampled weights
          lower      = estimate (the weights not sampled never fail)
          upper      = estimate + (1 - covered) (they always fail)
          estimate_z, estimate_x, std_error_z, std_error_x   the same per sector."""
        shape = np.shape(p)
        run = self.trials > 0
        B = binomial_pmf(self.n_locs, self.weights[run], p)
        n = self.trials[run].astype(np.float64)
        out = {}
        for key, k in (("", self.failures), ("_z", self.failures_z), ("_x", self.failures_x)):
            k = k[run].astype(np.float64)
            q = (k + 1.0) / (n + 2.0)
            out["estimate" + key] = (B * (k / n)).sum(axis=1).reshape(shape)            # (row by row: a p gives the same value alone or in an array)
            out["std_error" + key] = np.sqrt((B * B * (q * (1.0 - q) / n)).sum(axis=1)).reshape(shape)
        covered = np.minimum(B.sum(axis=1), 1.0).reshape(shape)                 # (the pmf sums to 1 up to rounding: never a negative remainder)
        out.update(covered=covered, lower=out["estimate"], upper=out["estimate"] + (1.0 - covered))
        return out


def _sweep(plan, stream, n_locs, weights, cap, target_failures, batch, base_seed):
    """f_w for every weight on one plan: stratum w runs the trials (w << STRATUM_SHIFT) + 0, 1, ...; with target_failures, whole batches until that
    many failures or `cap` trials (a stratum has no reference-order prefix to honour: what was run is what is counted)."""
    rows = []
    try:
        for w in weights:
            plan.use_fixed_weight(int(w))
            begin, done = int(w) << STRATUM_SHIFT, 0
            tally = np.zeros(_lib.TALLY_SLOTS, np.int64)
            while done < cap:
                count = cap - done if target_failures is None else min(batch, cap - done)
                plan.run(base_seed, begin + done, count, stream.ptr)
                tally += plan.read(stream.ptr, clear=True)
                done += count
                if target_failures is not None and tally[T["total_err"]] >= target_failures:
                    break
            rows.append((int(tally[T["trials"]]), int(tally[T["total_err"]]), int(tally[T["z_err"]]), int(tally[T["x_err"]]),
                         int(tally[T["bp_conv_z"]]), int(tally[T["bp_conv_x"]])))
    finally:
        plan.use_fixed_weight(None)
    rows = np.array(rows, np.int64).reshape(len(weights), 6)
    return WeightStrata(n_locs, weights, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4:6])


def _refuse_erasure(who, erasure):
    if erasure is not None:
        raise ValueError(f"{who}: erasure=... does not go with fixed-weight sampling (a weight stratum counts the faults of the independent draws alone)")


def _refuse_noise_model(who, noise_model):
    if noise_model is not None:
        raise ValueError(f"{who}: noise_model=... does not go with fixed-weight sampling (the weight strata reweight one rate p for every location)")


def _refuse_soft(who, soft):
    if soft is not None:
        raise ValueError(f"{who}: soft=... does not go with fixed-weight sampling (a weight stratum counts the faults of the independent draws alone)")


def run_weight_strata(Hx, Hz, Lx, Lz, prior_error_rate, weights=None, p_range=None, trials_per_weight=4096, target_failures=None,
                      max_trials_per_weight=None, coverage=1e-9, num_cycles=12, maxIter=50, decoder="bp_osd", osd_order=0, window=None, schedule="flooding",
                      layers=None, decimation=None, precision="f64", relay_params=None, precomputed_matrices=None, device=None, base_seed=0, batch=16384,
                      flags=0, lsd=None, erasure=None, noise_model=None, soft=None, **bb_params):
    """One sweep over the number of faults on the circuit plan of ``run_simulation`` -> WeightStrata.

    The circuit and decoder arguments are ``run_simulation``'s, under the same rules (``engine._extension_rules``: ValueError before any device call).
    ``prior_error_rate`` is the p the decoding matrices and priors are built at; the decoder is held fixed across the sweep, so f_w belongs to that
    decoder configuration.  Alpha is the dynamical schedule (the alpha / SCOPT estimators draw at one error rate and are not offered here), and
    ``osd_order > 0`` with ``decoder="bp_osd"`` (the reference's OSD-w pass, which runs outside the plan) raises ValueError.

    Which weights run: ``weights`` (an iterable of distinct fault counts), or ``p_range=(p_lo, p_hi)`` with ``coverage``: the contiguous range from the
    ``coverage`` quantile of Binomial(N, p_lo) to the ``1 - coverage`` quantile of Binomial(N, p_hi) (``weights_for``).
    Per weight: ``trials_per_weight`` trials; with ``target_failures``, batches of ``batch`` until that many failures or ``max_trials_per_weight``
    (default ``trials_per_weight``) trials -- whole batches, all counted.
    One plan on a single ``device`` serves the whole sweep; weight w uses the global trial range starting at ``w << 40``.
    ``erasure=...`` and ``soft=...`` raise ValueError: a weight counts the faults of the independent draws alone, and the plan refuses both beside it.
    ``noise_model=...`` raises ValueError too: LER(p) is rebuilt from the strata with one rate p for every location, and the plan refuses a model beside a weight."""
    _refuse_erasure("run_weight_strata", erasure)
    _refuse_soft("run_weight_strata", soft)
    _refuse_noise_model("run_weight_strata", noise_model)
    rules = engine._extension_rules(osd_order, precision, decimation, schedule, layers, window, decoder, relay_params, None, None, True, False, maxIter, None, lsd=lsd)
    if decoder == "bp_osd" and osd_order > 0:
        raise ValueError(f"osd_order={osd_order} with decoder='bp_osd' asks for the OSD-w pass, which runs outside the plan; use decoder='bp_osd_cs' "
                         "(osd_order is then the combination-sweep order)")
    if not 0.0 < float(prior_error_rate) < 1.0:
        raise ValueError("prior_error_rate must be in (0, 1)")
    weights, cap = _check_sweep_args(weights, p_range, coverage, trials_per_weight, target_failures, max_trials_per_weight, batch)
    dev = 0 if device is None else int(device)
    prob = engine._circuit_problem(Hx, Hz, Lx, Lz, prior_error_rate, num_cycles, precomputed_matrices, dev, bb_params)
    ws = _resolve_weights(np.asarray(prob.compiled.base_ops).size, weights, p_range, coverage)
    switch, _ = engine._plan_switch(rules, [(g.indptr, g.indices, g.n) for g in prob.graphs], osd_order)
    plan = prob.make_plan(prob.graphs, maxIter, 1.0, 1.0, "dynamical", batch, flags)
    stream = _lib.Stream(dev)
    try:
        switch(plan)
        return _sweep(plan, stream, plan.n_locs, ws, cap, target_failures, int(batch), int(base_seed))
    finally:
        plan.close()
        stream.close()


def run_dem_weight_strata(dem, weights=None, p_range=None, trials_per_weight=4096, target_failures=None, max_trials_per_weight=None, coverage=1e-9,
                          maxIter=50, decoder="bp_osd", osd_order=0, window=None, schedule="flooding", layers=None, decimation=None, precision="f64",
                          relay_params=None, alpha_mode=None, alvarado_alpha=None, device=None, base_seed=0, batch=16384, flags=0, lsd=None, erasure=None, soft=None):
    """``run_weight_strata`` for a DetectorErrorModel whose mechanisms all have ONE probability (N = its mechanisms); the arguments and rules are
    ``run_dem_simulation``'s.  The decoder view -- and with it the priors -- is the model's own, held fixed across the sweep.  A model with two
    different probabilities raises ValueError before any device call, and so do ``erasure=...`` and ``soft=...``."""
    _refuse_erasure("run_dem_weight_strata", erasure)
    _refuse_soft("run_dem_weight_strata", soft)
    rules, alpha_mode, alphas = dem_mod._dem_rules("run_dem_weight_strata", dem, maxIter, osd_order, alpha_mode, alvarado_alpha, decoder, relay_params, window,
                                                   schedule, layers, decimation, precision, lsd=lsd)
    thr = np.floor(dem.prob * 4294967296.0)
    odd = np.flatnonzero(thr != thr[0]) if thr.size else np.zeros(0, np.int64)
    if odd.size:
        raise ValueError(f"mechanism {int(odd[0])} has probability {dem.prob[odd[0]]!r}, mechanism 0 has {dem.prob[0]!r}: weight strata need one "
                         "probability for all mechanisms")
    weights, cap = _check_sweep_args(weights, p_range, coverage, trials_per_weight, target_failures, max_trials_per_weight, batch)
    ws = _resolve_weights(dem.n_mech, weights, p_range, coverage)
    dev = 0 if device is None else int(device)
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    switch, _ = engine._plan_switch(rules, [(v.indptr, v.indices, v.shape[1]) for v in views], osd_order)
    graphs = [_lib.Graph(v.indptr, v.indices, v.shape[1], device=dev) for v in views]
    plan = dem.plan(graphs, max_iter=maxIter, alphas=alphas, alpha_mode=alpha_mode, batch=batch, flags=flags)
    stream = _lib.Stream(dev)
    try:
        switch(plan)
        return _sweep(plan, stream, dem.n_mech, ws, cap, target_failures, int(batch), int(base_seed))
    finally:
        plan.close()
        stream.close()
