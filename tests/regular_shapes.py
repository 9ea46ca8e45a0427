"""Seeded cases for the regular min-sum kernel (csrc/minsum_regular.hip) over the whole domain its entry points accept: every team size plan_regular
takes (S = 14 .. 1, a block that ends in the middle of a wave, the 512-thread limit and the first graph beyond it), clean priors of every kind
(inputs_clean of csrc/decode_api.hip: finite and not -0.0), and batches large enough that a workgroup of the persistent grid takes a second `base`.
tests/test_regular_domain_cpu.py checks with the oracle alone that the cases have the properties they are named for;
tests/test_regular_domain_gpu.py decodes them.  Plain module (no pytest hooks); deterministic from the seeds below.

The graphs come from graph_shapes.deal (configuration model, row_cap = check degree); each seed below gives an exactly regular graph, which graph()
asserts.  `rate` is the error rate of the random errors behind the syndromes, chosen per graph so that min-sum both converges and fails on them
(at m = 512 a rate of 0.03 converges on every shot)."""
from types import SimpleNamespace

import numpy as np

import graph_shapes as GS

SEED = 20261018
GRID_CAP = 3072                 # persistent_grid of csrc/minsum_regular.hip: 256 * 12 workgroups
LB_T = 512                      # QLDPC_LB_T: the largest team, and the thread budget S = LB_T / TS is cut from
CLIPS = (20.0, 6.0, 1.0)
MAX_ITER = 50
PRIOR_SHOTS, TEAM_SHOTS = 256, 64
FIRST_ITERATION_BYTES = 60 * 1024          # qldpc_cc_plan_create: (m + n) * 64 <= 60 KiB for the bit-sliced first iteration

# name: (check degree, variable degree, m, error rate of the syndromes, decoder form, what it reaches)
TABLE = {
    "r63_m36": (6, 3, 36, 0.04, "REGULAR", "S = 14: many shots per workgroup"),
    "r63_m256": (6, 3, 256, 0.055, "REGULAR", "S = 2; the block is exactly 2 * TS"),
    "r63_m257": (6, 3, 257, 0.055, "REGULAR", "S = 1, block 320: 63 lanes belong to no team"),
    "r63_m320": (6, 3, 320, 0.055, "REGULAR", "last graph inside the first-iteration pipeline's (m + n) * 64 bound"),
    "r63_m321": (6, 3, 321, 0.055, "REGULAR", "first graph beyond it"),
    "r63_m512": (6, 3, 512, 0.055, "REGULAR", "the largest team"),
    "r42_m512": (4, 2, 512, 0.04, "REGULAR", "the largest team, (4,2)"),
    "r84_m512": (8, 4, 512, 0.05, "REGULAR", "the largest team, (8,4): LDS above the 39 KiB target with S = 1"),
    "r63_m513": (6, 3, 513, 0.055, "RESIDENT", "not REGULAR any more"),
    "r84_m24": (8, 4, 24, 0.05, "REGULAR", "S cut back by the 39 KiB loop of plan_regular"),
    # small (4,2) graph for the Monte-Carlo plan (the decode API meets (4,2) at m = 512)
    "r42_m30": (4, 2, 30, 0.04, "REGULAR", "a small (4,2) team"),
}
TEAM_GRAPHS = ("r63_m36", "r63_m256", "r63_m257", "r63_m320", "r63_m321", "r63_m512", "r42_m512", "r84_m512", "r63_m513", "r84_m24")
PRIOR_GRAPHS = ("r63_m36", "r63_m257")
PRIOR_CLASSES = ("uniform", "normal", "negative class", "zero class", "above clip", "all zero", "subnormal", "huge")
MC_GRAPHS = ("r63_m36", "r42_m30", "r84_m24")
SECOND_TRIP = {"r63_m257": ("normal", 20.0), "r63_m36": ("zero class", 6.0)}      # graph: (prior class, clip) of its second-trip decode
# Monte-Carlo plan: error rates at and beyond 0.5 (prior +0.0, negative inside a clip of 1.0, negative outside it), the first-iteration pipeline's
# bound, and a call that sends the S = 1 graph's workgroups on a second trip with BP failures to export
MC_SEED, MC_SHOTS, MC_PS, MC_CLIPS = 20261018, 3000, (0.5, 0.7, 0.93), (20.0, 1.0)
MC_BOUND_P, MC_BOUND_SHOTS = 0.01, 3300
MC_TRIP_P, MC_TRIP_SHOTS = 0.05, GRID_CAP + 228
GRAPH_SALT = {"r63_m36": 1}     # the deal of the plain seed leaves one stub of this graph unplaced; the next seed is exactly regular

_GRAPHS = {}


def plan(cdeg, m, n, max_iter=MAX_ITER):
    """plan_regular of csrc/minsum_regular.hip restated -> (TS, S, block, LDS bytes), or None where it refuses (team or iteration table too large)"""
    ts = max(m, (n + 1) // 2)
    if ts > LB_T or max_iter > 1024:
        return None
    rst = cdeg + 1 if cdeg % 2 == 0 else cdeg
    nq = (n + 3) // 4

    def lds(s):
        off_e = s * m * rst * 8 + s * n * 8
        off_l = (off_e + s * nq * 4 + 7) // 8 * 8
        off_a = (off_l + s * 8 + (6 * s + 2) * 4 + 7) // 8 * 8
        return off_a + max(max_iter, 1) * 8 + 6 * 8 + 16
    S = LB_T // ts
    while S > 1 and lds(S) > 39 * 1024:
        S -= 1
    return ts, S, (S * ts + 63) // 64 * 64, lds(S)


def graph(name):
    """-> SimpleNamespace(name, cdeg, vdeg, m, n, indptr, indices, cols [m, cdeg], rate, expected, note, TS, S, block, lds)"""
    if name not in _GRAPHS:
        cdeg, vdeg, m, rate, expected, note = TABLE[name]
        assert m * cdeg % vdeg == 0
        n = m * cdeg // vdeg
        seed = [SEED, cdeg, m] + ([GRAPH_SALT[name]] if name in GRAPH_SALT else [])
        ip, ix = GS.deal(np.random.default_rng(seed), m, np.full(n, vdeg), row_cap=cdeg)
        rd, cd = GS.degrees(ip, ix, n)
        assert GS.regular_takes(rd, cd) and (int(rd.max()), int(cd.max())) == (cdeg, vdeg), name
        p = plan(cdeg, m, n)
        g = SimpleNamespace(name=name, cdeg=cdeg, vdeg=vdeg, m=m, n=n, indptr=ip, indices=ix, cols=ix.reshape(m, cdeg).astype(np.int64), rate=rate,
                            expected=expected, note=note, TS=None, S=None, block=None, lds=None)
        if p:
            g.TS, g.S, g.block, g.lds = p
        _GRAPHS[name] = g
    return _GRAPHS[name]


def _rng(g, *what):
    return np.random.default_rng([SEED, g.cdeg, g.m] + [int(w) for w in what])


def overflow_column(g):
    """The column of the `huge` class whose three checks have huge priors on every other edge: the unclipped messages of iteration 0 into it are
    alpha_0 * 1.5e308 each, and their sum overflows."""
    return int(_rng(g, 8).integers(0, g.n))


def priors(g):
    """The prior classes, every one clean by inputs_clean (finite, no -0.0) -> {class name: f64 [n]}"""
    n = g.n
    base = np.log((1 - g.rate) / g.rate)
    nine, seven = max(1, n // 9), max(1, n // 7)
    out = {"uniform": np.full(n, base),
           "normal": base + _rng(g, 1).normal(0.0, 0.5, n),
           "negative class": GS.by_class(_rng(g, 2), n, [-1.5, 4.0], sizes=[nine, n - nine]),
           "zero class": GS.by_class(_rng(g, 3), n, [0.0, 4.0], sizes=[nine, n - nine]),
           "above clip": GS.by_class(_rng(g, 4), n, [27.0, 4.0], sizes=[seven, n - seven]),
           "all zero": np.zeros(n),
           "subnormal": GS.by_class(_rng(g, 5), n, [5e-324, 1e-310, 3.0], sizes=[3, 3, n - 6])}
    # huge: 1.5e308 on the other columns of the checks of one column (at most vdeg * (cdeg - 1) of them), 4.0 on the rest
    huge = np.full(n, 4.0)
    j = overflow_column(g)
    rows = np.flatnonzero((g.cols == j).any(axis=1))
    huge[np.setdiff1d(g.cols[rows].ravel(), [j])] = 1.5e308
    out["huge"] = huge
    assert list(out) == list(PRIOR_CLASSES)
    return out


def syndromes_of(g, errors):
    return (np.asarray(errors, np.int64)[:, g.cols].sum(axis=-1) & 1).astype(np.int8)


SCALES = (0.25, 0.5, 1.0, 1.5)


def syndromes(g, B, prior=None, salt=0):
    """B syndromes of random errors, then (B >= 2) an all-zero one last and (B >= 3) an unrealisable (random) one first, as graph_shapes.syndromes has
    them, and (B >= 4, with a prior) second the syndrome of the error that the prior's signs state (e[j] = prior[j] < 0): with a clip of 1 and a
    negative class on a ninth of 514 columns it is the only kind of shot that converges.  Even shots draw every bit with probability g.rate times SCALES[(b / 2) % 4], so that easy and hard shots alternate; odd shots draw bit j
    with the probability its prior states, 1 / (1 + exp(prior[j])) (g.rate without a prior), so that a negative class has the errors it announces."""
    rng = _rng(g, 7, salt, B)
    q = np.full((B, g.n), g.rate) * np.asarray(SCALES)[(np.arange(B) // 2) % 4][:, None]
    if prior is not None:
        with np.errstate(over="ignore"):
            q[1::2] = 1.0 / (1.0 + np.exp(np.asarray(prior, np.float64)))
    else:
        q[1::2] = g.rate
    S = syndromes_of(g, rng.random((B, g.n)) < q)
    if B >= 3:
        S[0] = rng.random(g.m) < 0.5
    if B >= 4 and prior is not None:
        S[1] = syndromes_of(g, (np.asarray(prior) < 0)[None, :])[0]
    if B >= 2:
        S[-1] = 0
    return S


def logicals(g, k=3):
    """k random rows over the columns: what the Monte-Carlo plan compares e xor e_hat against (any k x n matrix serves)"""
    return (_rng(g, 9).random((k, g.n)) < 0.5).astype(np.uint8)


# ---------------------------------------------------------------------------------------- the decode cases of the GPU module
def decode_cases():
    """Every decode the GPU module runs against the oracle -> list of SimpleNamespace(id, graph, prior (class name), clip, B, max_iter, alpha_mode, alpha,
    damping, salt, modelled).  modelled: tests/loo_messages_model.py covers it (dynamical alpha, no damping)."""
    out = []

    def add(kind, gname, prior, clip, B, max_iter=MAX_ITER, alpha_mode="dynamical", alpha=1.0, damping=1.0, salt=0):
        out.append(SimpleNamespace(id=f"{kind}-{gname}-{prior.replace(' ', '_')}-clip{clip:g}", kind=kind, graph=gname, prior=prior, clip=clip, B=B,
                                   max_iter=max_iter, alpha_mode=alpha_mode, alpha=alpha, damping=damping, salt=salt,
                                   modelled=(alpha_mode == "dynamical" and damping == 1.0)))
    for gname in PRIOR_GRAPHS:
        for prior in PRIOR_CLASSES:
            for clip in CLIPS:
                add("prior", gname, prior, clip, PRIOR_SHOTS)
    for gname in TEAM_GRAPHS:
        for prior in ("uniform", "normal"):
            add("team", gname, prior, 20.0, TEAM_SHOTS, salt=1)
    for gname in PRIOR_GRAPHS:
        add("const", gname, "negative class", 6.0, PRIOR_SHOTS, alpha_mode="alvarado", alpha=0.8)
        add("seq", gname, "negative class", 6.0, PRIOR_SHOTS, alpha_mode="alvarado-autoregressive", alpha=np.array([0.55, 0.7, 0.9]))
        add("damped", gname, "normal", 6.0, PRIOR_SHOTS, damping=0.85)
    assert len({c.id for c in out}) == len(out)
    return out


NEVER_CONVERGE = 16             # shots of the iteration-cap case


def never_converging(g, oracle, prior, count=NEVER_CONVERGE, max_iter=1025):
    """`count` syndromes on which the oracle does not converge within max_iter iterations: unrealisable ones (random bits), kept where the oracle says so"""
    rng = _rng(g, 11)
    S = (rng.random((4 * count, g.m)) < 0.5).astype(np.int8)
    conv = np.asarray(oracle.minsum_decode_batch(g.indptr, g.indices, g.n, S, prior, max_iter=max_iter, threads=0)[1]).astype(bool)
    keep = np.flatnonzero(~conv)[:count]
    assert len(keep) == count
    return S[keep]


# ---------------------------------------------------------------------------------------- second trip of the persistent loop
def second_trip(name):
    """-> (graph, B, trips): a batch that sends workgroups on a second `base`; trips = [(shot of the first trip, shot of the second trip)] for every
    (workgroup, slot) that decodes twice"""
    g = graph(name)
    extra = 128 if g.S == 1 else g.S + 3                   # S > 1: one full second group and a ragged one (3 of its S slots hold a shot)
    B = GRID_CAP * g.S + extra
    return g, B, [(b - GRID_CAP * g.S, b) for b in range(GRID_CAP * g.S, B)]
