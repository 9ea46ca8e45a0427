"""One chain for every (path, OSD stage) pair of a circuit or DEM plan: the plan's answer built from the C ABI's batch entry points piece by piece --
the BP stage of the path per sector, the OSD stage on the BP failures, and the judge in numpy.  Each batch entry point used here is pinned to its own
numpy model in its own module; nothing in chain() calls a CircuitPlan method (sample_for() wraps the samplers, switch_path() moves the plan under
test).  The pairs themselves, and switch_allowed's rule restated as a predicate, are at the top: tests/test_plan_pairs_cpu.py checks the one against
the other and tests/test_plan_pairs_gpu.py parametrises over them.  Plain module: no pytest hooks, no device call at import."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsd_stats_model as SM  # noqa: E402

# ---------------------------------------------------------------------------------------- the two axes and their rule
# path -> the display name in the library's messages (switch_allowed's path_name) and in include/qldpc_hip.h
PATH_NAMES = {"flooding": "flooding", "layered": "the layered schedule", "decimation": "guided decimation", "f32": "f32", "relay": "Relay-BP",
              "window": "windows", "correlated": "correlated decoding", "erasure_aware": "erasure-aware decoding", "soft_aware": "soft-aware decoding"}
PATHS = tuple(PATH_NAMES)
STAGES = ("osd0", "osd_cs", "lsd")
WITHOUT_STAGE_SWITCH = ("relay", "window")                                  # the paths that go with neither OSD-CS nor LSD
# the cases of the GPU module: a path, or a path with the mode of its links
LSD_CASES = ("layered", "decimation", "f32", "correlated:raise", "correlated:condition", "erasure_aware", "soft_aware")
ALL_CASES = ("flooding",) + LSD_CASES
KINDS = ("cols_1", "llr_2", "llr_inf")                                     # the confidence kinds of the GPU module: a sum, a sum of squares and a max
ALPHA = {"correlated:raise": 1.0, "correlated:condition": 0.875, "erasure_aware": 1.0, "soft_aware": 0.875}      # the constant alpha of the per-shot-prior paths


def path_of(case):
    return case.split(":")[0]


def allowed(path, stage, use_osd=True, damping=1.0, confidence=False):
    """switch_allowed (csrc/circuit.hip) for a plan that ends on `path` with `stage`, whichever switch came first: OSD-CS and LSD need use_osd and go
    with every path but Relay-BP and windows; windows need use_osd as well; every path but flooding and Relay-BP needs damping = 1; a confidence rides
    on LSD."""
    if stage != "osd0" and (not use_osd or path in WITHOUT_STAGE_SWITCH):
        return False
    if path == "window" and not use_osd:
        return False
    if damping != 1.0 and path not in ("flooding", "relay"):
        return False
    return stage == "lsd" or not confidence


# ---------------------------------------------------------------------------------------- the plan under test
def context(L, name):
    """Everything a case needs of a shape, once: "hgp" of tests/circuit_shapes.py (tables from the MODEL's signatures, as aware_setup builds them) or
    "circ72" (the feature modules' setups).  -> namespace(compiled, Lx, Lz, p, graphs, masks, priors, soft_priors, era, soft, links, readout)"""
    if name in _CONTEXTS:
        return _CONTEXTS[name]
    from test_soft_gpu import channels
    if name == "circ72":
        import test_correlated_gpu as TCO
        import test_erasure_gpu as TE
        import test_soft_gpu as TS
        c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = TS.setup(L)
        ctx = SimpleNamespace(compiled=compiled, Lx=c["Lx"], Lz=c["Lz"], p=TS.P, graphs=graphs, masks=masks, priors=priors, soft_priors=marg["gaussian"],
                              era=TE.setup(L)[9], soft=tables["gaussian"], links={m: TCO.circuit_links(L, m) for m in ("raise", "condition")})
    else:
        import test_circuit_shapes_cpu as TC
        import test_circuit_shapes_gpu as TG
        S, sigs, M, graphs, priors, masks, plan = TG.setup(L, name)
        era, soft, marg, links = TG.aware_setup(L, name)
        ctx = SimpleNamespace(compiled=S.compiled, Lx=S.Lx, Lz=S.Lz, p=TC.P_LOW, graphs=graphs, masks=masks, priors=priors, soft_priors=marg, era=era, soft=soft,
                              links=links)
    ctx.name, ctx.readout = name, channels()["gaussian"]
    _CONTEXTS[name] = ctx
    return ctx


_CONTEXTS = {}


def priors_of(ctx, case):
    """the priors a plan of this case is created with: the marginal priors of the readout channel on the soft-aware path (matched priors)"""
    return ctx.soft_priors if case == "soft_aware" else ctx.priors


def make_plan(L, ctx, case, batch, p=None, **kw):
    pr = priors_of(ctx, case)
    return L.CircuitPlan(ctx.compiled, ctx.Lx, ctx.Lz, ctx.graphs[0], ctx.graphs[1], pr[0], pr[1], ctx.masks[0], ctx.masks[1], ctx.p if p is None else p,
                         batch=batch, **kw)


def switch_path(plan, ctx, case, decim=None, rates=None):
    """the path switch of a case, and the sampler that feeds it its per-shot priors"""
    path = path_of(case)
    if path == "layered":
        plan.use_layered()
    elif path == "decimation":
        plan.use_decimation(**decim)
    elif path == "f32":
        plan.use_f32()
    elif path == "correlated":
        lk = ctx.links[case.split(":")[1]]
        plan.use_correlated(ALPHA[case], lk, lk.base)
    elif path == "erasure_aware":
        plan.use_erasure_aware(ALPHA[case], ctx.era)
        plan.use_erasure_noise(rates)
    elif path == "soft_aware":
        plan.use_soft_aware(ALPHA[case], ctx.soft)
        plan.use_soft_readout(ctx.readout)
    else:
        assert path == "flooding", case


def sample_for(plan, case, seed, begin, count):
    """the plan's own sampler -> (syndromes per sector, truths per sector, per-shot priors per sector or None)"""
    if case == "erasure_aware":
        spz, tz, spx, tx, _, pz, px = plan.sample_erasures(seed, begin, count, want_priors=True)
        return (spz, spx), (tz, tx), (pz, px)
    if case == "soft_aware":
        spz, tz, spx, tx, _, pz, px = plan.sample_soft(seed, begin, count, want_priors=True)
        return (spz, spx), (tz, tx), (pz, px)
    spz, tz, spx, tx = plan.sample(seed, begin, count)
    return (spz, spx), (tz, tx), None


# ---------------------------------------------------------------------------------------- the chain
def bp_stage(L, case, g, synd, prior, max_iter, decim=None, links=None, src_err=None):
    """the BP stage of a path on one sector -> (det, conv, llr, iterations as the tally counts them, legs or None, extra): extra is the prior per shot
    on a per-shot-prior path, the number of frozen columns per shot after guided decimation, else None.
    prior: f64[n], or f64[B, n] on a per-shot-prior path.  The judge adds one iteration per trial; the decimation and per-shot-prior launches are
    given a bias of -1 (decode_sector), so their slots hold the iterations themselves."""
    path = path_of(case)
    if path == "flooding":
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, max_iter, "dynamical", 1.0)
        return det, conv, llr, iters.astype(np.int64) + 1, None, None
    if path in ("layered", "f32"):
        dec = (L.LayeredDecoder if path == "layered" else L.Minsum32Decoder)(g, prior, max_iter=max_iter)
        det, conv, llr, iters = dec.decode(synd)
        dec.close()
        return det, conv, llr, iters.astype(np.int64) + 1, None, None
    if path == "decimation":
        det, llr, conv, iters, rounds, fixed = L.decim_decode_batch(g, synd, prior, clip_llr=20.0, **decim)
        return det, conv, llr, iters.astype(np.int64), rounds.astype(np.int64), fixed
    kw = dict(links=links, src_err=src_err) if links is not None else {}
    det, llr, conv, iters, used = L.shotprior_decode_batch(g, synd, prior, ALPHA[case], 20.0, max_iter, want_prior=True, **kw)
    return det, conv, llr, iters.astype(np.int64), None, used


def osd_stage(L, g, synd, det, llr, conv, stage, prior, cs_order=None, lsd=None, weights=None):
    """the OSD stage on the BP failures, in place in `det` -> (info int32[failures, 4] or None, stats uint64[B, 8]: eight zeros for a converged row)"""
    bad = np.flatnonzero(conv == 0)
    stats, info = np.zeros((synd.shape[0], 8), np.uint64), None
    if stage == "lsd":
        info = np.zeros((0, 4), np.int32)
    if bad.size == 0:
        return info, stats
    if stage == "osd0":
        det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
    elif stage == "osd_cs":
        det[bad] = L.osdcs_batch(g, synd[bad], llr[bad], det[bad], prior, cs_order)[0]      # the plan's prior scores, on every path
    else:
        det[bad], info, stats[bad] = L.lsd_stats_batch(g, synd[bad], llr[bad], det[bad], lsd[0], lsd[1], weights)
    return info, stats


def chain(L, graphs, priors, synds, case, stage, max_iter=50, shot_priors=None, decim=None, links=None, cs_order=None, lsd=None, stale_links=False):
    """A batch through the pieces, sector by sector: the BP stage of the path, then the OSD stage on its failures.  Correlated decoding: sector 1 reads
    its links against sector 0's FINISHED correction (stale_links: against the BP stage's, a mutant that must not equal the plan); its prior is
    links.base where there is one.  shot_priors: f64[B, n] per sector from the sampler (None: the plan's prior for every shot, which is also what a
    plan does with recorded events).  The weights of the statistics are quantise_weights of the plan's priors.
    -> namespace with a list per sector of det, conv, llr (as handed over), handed (det as handed over), iters, legs, info, stats, flags, and
    used_prior (per-shot-prior paths) or fixed (guided decimation)"""
    out = SimpleNamespace(det=[], conv=[], llr=[], handed=[], iters=[], legs=[], info=[], stats=[], used_prior=[], fixed=[])
    for s, (g, synd) in enumerate(zip(graphs, synds)):
        prior, kw = priors[s] if shot_priors is None else shot_priors[s], {}
        if path_of(case) == "correlated" and s == 1:
            prior = priors[1] if links.base is None else links.base
            kw = dict(links=links, src_err=out.handed[0] if stale_links else out.det[0])
        det, conv, llr, iters, legs, extra = bp_stage(L, case, g, synd, prior, max_iter, decim, **kw)
        used, fixed = (None, extra) if path_of(case) == "decimation" else (extra, None)
        out.handed.append(det.copy())
        info, stats = osd_stage(L, g, synd, det, llr, conv, stage, priors[s], cs_order, lsd, L.quantise_weights(priors[s]))
        for name, v in (("det", det), ("conv", conv), ("llr", llr), ("iters", iters), ("legs", legs), ("info", info), ("stats", stats), ("used_prior", used),
                        ("fixed", fixed)):
            getattr(out, name).append(v)
    out.flags = np.zeros((2, 3), np.int64)
    for s, info in enumerate(out.info):
        if info is not None and info.shape[0]:
            out.flags[s] = np.bincount(info[:, 0], minlength=3)
    return out


# ---------------------------------------------------------------------------------------- the judge
def predictions(res, masks):
    """uint64[B] per sector: the logical bits of the chain's corrections (bit r = observable r)"""
    from test_correlated_gpu import logical_bits
    return [logical_bits(d, masks[s]) for s, d in enumerate(res.det)]


def outcomes(res, masks, truths):
    """uint8[B]: bit s = sector s's correction differs from the truth in some logical"""
    from test_erasure_gpu import verdicts
    return verdicts(masks, res.det, truths)


def expected_tally(L, res, outcome):
    """{slot name: value} of the slots a path fills: the trials and error slots, and per sector the BP successes, an OSD call per failure, the
    iterations, and the summed rounds of guided decimation (0 elsewhere)"""
    want = {"trials": outcome.size, "z_err": int(np.count_nonzero(outcome & 1)), "x_err": int(np.count_nonzero(outcome & 2)), "total_err": int(np.count_nonzero(outcome))}
    for s in range(len(res.det)):
        sfx = "zx"[s]
        want["bp_conv_" + sfx] = int(res.conv[s].sum())
        want["osd_" + sfx] = int((res.conv[s] == 0).sum())
        want["iters_" + sfx] = int(res.iters[s].sum())
        want["legs_" + sfx] = int(res.legs[s].sum()) if res.legs[s] is not None else 0
    return want


def assert_tally(L, tally, want):
    got = {name: int(tally[L.TALLY[name]]) for name in want}
    assert got == want, {name: (got[name], want[name]) for name in want if got[name] != want[name]}


def scores(kind, res):
    """lsd_stats_model.scores on the chain's statistics (a one-sector chain: sector X contributes zeros)"""
    return SM.scores(kind, res.stats[0], res.stats[1] if len(res.stats) == 2 else None)
