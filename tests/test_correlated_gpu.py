"""Two-pass correlated decoding on a circuit plan (qldpc_circuit_plan_use_correlated), on circ72 -- the small plan of tests/test_plan_switch_gpu.py -- and
on the toy model of tests/correlated_model.py: the plan equals the chain of its parts verdict for verdict, recorded events ride along, the toy model's
verdict turns, the switch rules gain one row and one column, and run_simulation / run_dem_simulation equal the plan driven by hand."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402
from test_plan_switch_gpu import BASE_SWITCHES as SWITCHES, refused, run64, BATCH  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, COUNT = 2031, 384
_LINKS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def circuit_links(L, mode="raise"):
    """links_from_circuit on circ72 at the plan's p = 0.005, once per mode"""
    if mode not in _LINKS:
        from qldpc_amd.simulation.correlated import links_from_circuit
        c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
        _LINKS[mode] = links_from_circuit(compiled, c["Lx"], c["Lz"], M, 0.005, mode=mode)
    return _LINKS[mode]


def logical_bits(det, mask):
    """uint64[B]: XOR of the logical masks of a correction's ones"""
    out = np.zeros(det.shape[0], np.uint64)
    for b in range(det.shape[0]):
        for v in mask[np.flatnonzero(det[b])]:
            out[b] ^= v
    return out


def chain(L, graphs, priors, masks, synd, alpha, links, base, max_iter=50, osd=None):
    """sector 0 -> its OSD stage on the unconverged -> sector 1 with the links against sector 0's correction -> its OSD stage.  -> (det, conv) per sector"""
    out = []
    for s in range(2):
        kw = dict(links=links if links is not None else (np.zeros(graphs[1].n + 1, np.int32), [], []), src_err=out[0][0]) if s == 1 else {}
        prior = base if (s == 1 and base is not None) else priors[s]
        det, llr, conv, _ = L.shotprior_decode_batch(graphs[s], synd[s], prior, alpha, 20.0, max_iter, **kw)
        failed = np.flatnonzero(conv == 0)
        if failed.size:
            if osd is None:
                det[failed] = L.osd0_batch(graphs[s], synd[s][failed], llr[failed], det[failed])
            else:
                det[failed] = L.osdcs_batch(graphs[s], synd[s][failed], llr[failed], det[failed], priors[s], osd)[0]      # the shared prior scores: the documented limitation
        out.append((det, conv))
    return out


# ---------------------------------------------------------------------------------------- 1. composition, 2. events
def test_links_of_the_circuit(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    lk = circuit_links(L)
    assert lk.n == graphs[1].n and lk.n_src == graphs[0].n and lk.n_links > graphs[1].n // 2 and lk.unmatched == 0 and lk.base is None
    assert (np.diff(lk.ptr) >= 0).all() and lk.src.min() >= 0 and lk.src.max() < graphs[0].n and np.isfinite(lk.llr).all()
    for j in np.flatnonzero(np.diff(lk.ptr) > 1)[:50]:
        assert (np.diff(lk.src[lk.ptr[j]:lk.ptr[j + 1]]) > 0).all()
    cond = circuit_links(L, "condition")
    assert cond.base is not None and np.array_equal(cond.src, lk.src) and (cond.base >= priors[1] - 1e-9).all()      # U_j <= the column's whole mass


@pytest.mark.parametrize("how", ["raise", "condition", "none", "raise+osd_cs"])
def test_the_plan_equals_the_chain_of_its_parts(L, how):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    links = None if how == "none" else circuit_links(L, how.split("+")[0])
    base = None if links is None else links.base
    alpha = 0.875 if how == "condition" else 1.0
    p = plan(batch=128)                                                    # three batches
    if how.endswith("osd_cs"):
        p.use_osd_cs(5)
    p.use_correlated(alpha, links, base)
    got = p.run_outcomes(SEED, 0, COUNT)
    tally = p.read(clear=True)
    spz, tz, spx, tx = p.sample(SEED, 0, COUNT)
    (dz, cz), (dx, cx) = chain(L, graphs, priors, masks, (spz, spx), alpha, links, base, osd=5 if how.endswith("osd_cs") else None)
    k = tz.shape[1]
    truth = [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in (tz, tx)]
    pz, px = logical_bits(dz, masks[0]), logical_bits(dx, masks[1])
    want = (pz != truth[0]).astype(np.uint8) | ((px != truth[1]).astype(np.uint8) << 1)
    assert np.array_equal(got, want), how
    T = L.TALLY
    assert tally[T["trials"]] == COUNT and tally[T["bp_conv_z"]] == cz.sum() and tally[T["bp_conv_x"]] == cx.sum()
    assert tally[T["osd_z"]] == COUNT - cz.sum() and tally[T["osd_x"]] == COUNT - cx.sum() and tally[T["legs_z"]] == 0 and tally[T["legs_x"]] == 0
    assert 0 < cz.sum() < COUNT                                            # both stages took part
    # recorded events: the same predictions from the packed syndromes
    pred0, pred1, flags = p.decode_events(L.pack_events(np.hstack([spz, spx])))
    assert np.array_equal(pred0, pz) and np.array_equal(pred1, px)
    assert np.array_equal(flags & 1, cz) and np.array_equal((flags >> 1) & 1, cx)
    p.close()


def test_the_links_change_sector_x_only(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    outs = {}
    for how in ("none", "raise"):
        p = plan(batch=128)
        p.use_correlated(1.0, None if how == "none" else circuit_links(L))
        outs[how] = p.run_outcomes(SEED, 0, COUNT)
        p.close()
    assert np.array_equal(outs["none"] & 1, outs["raise"] & 1)


# ---------------------------------------------------------------------------------------- 3. the toy model end to end
def test_toy_model_end_to_end(L):
    from qldpc_amd.simulation.dem import DemDecoder
    toy = CM.toy_dem()
    record = np.array([[1, 0, 1, 0]], np.uint8)                            # {a0, d0}: mechanism A fired
    for alpha in (1.0, 0.875):
        dec = DemDecoder(toy, correlated={"alpha": alpha})
        p0, p1 = dec.decode_batch(record)
        assert p0.tolist() == [[False]] and p1.tolist() == [[True]]        # the observable flip is predicted
        dec.close()
    plain = DemDecoder(toy)
    assert plain.decode_batch(record)[1].tolist() == [[False]]             # without the links sector 1 picks B
    plain.close()
    nolinks = DemDecoder(toy, correlated={"alpha": 1.0})
    nolinks._rules.links = None                                            # the path alone, nothing to raise
    assert nolinks.decode_batch(record)[1].tolist() == [[False]]
    nolinks.close()


# ---------------------------------------------------------------------------------------- 4. switch rules
ALL = dict(SWITCHES, lsd=("BP + LSD", lambda p: p.use_lsd(), lambda p: p.use_lsd(max_rows=128)))
CORR = ("correlated decoding", lambda p: p.use_correlated(), lambda p: p.use_correlated(0.875))
GOES_WITH = {"osd_cs", "lsd"}


def test_the_new_row_and_column_of_the_switch_table(L):
    plan = circuit_setup(L, "circ72")[6]
    assert len(ALL) == 7
    for other, (name, call, _) in ALL.items():
        p = plan(batch=BATCH)                                              # the row: correlated first
        CORR[1](p)
        if other in GOES_WITH:
            call(p)
            run64(L, p)
        else:
            refused(L, p, call, CORR[0], name)
        p.close()
        p = plan(batch=BATCH)                                              # the column: correlated second
        call(p)
        if other in GOES_WITH:
            CORR[1](p)
            run64(L, p)
        else:
            refused(L, p, CORR[1], name, CORR[0])
        p.close()


def test_asked_again_one_sector_damping_and_no_osd(L):
    plan = circuit_setup(L, "circ72")[6]
    p = plan(batch=BATCH)
    CORR[1](p)
    a = p.run_outcomes(7, 0, BATCH)
    CORR[2](p)                                                             # again: new arguments
    p.use_correlated(0.875, circuit_links(L))
    b = p.run_outcomes(7, 0, BATCH)
    p.use_correlated()
    assert np.array_equal(p.run_outcomes(7, 0, BATCH), a) and a.shape == b.shape
    lk = circuit_links(L)
    p.read(clear=True)                                                     # (run_outcomes tallies too)
    before = run64(L, p)
    for bad, text in (((lk.ptr, lk.src[::-1].copy(), lk.llr), "link_src["), ((lk.ptr, lk.src + p.graph_z.n, lk.llr), "link_src["),
                      ((lk.ptr, lk.src, np.full(lk.n_links, np.inf)), "link_llr[0]")):
        with pytest.raises(L.QldpcError, match="error -1") as ei:
            p.use_correlated(1.0, bad)
        assert text in str(ei.value)
    with pytest.raises(L.QldpcError, match=r"error -1: .*base_x\[3\]"):
        p.use_correlated(1.0, None, np.where(np.arange(p.graph_x.n) == 3, np.nan, 1.0))
    with pytest.raises(ValueError):
        p.use_correlated(0.0)
    assert np.array_equal(run64(L, p), before)
    p.close()
    p = plan(batch=BATCH, damping=0.5)
    refused(L, p, CORR[1], CORR[0], "damping = 1", reason="damping")
    p.close()
    p = plan(batch=BATCH, use_osd=False)                                   # BP alone: no OSD stage is needed
    CORR[1](p)
    t = run64(L, p)
    assert t[L.TALLY["osd_z"]] == 0 and t[L.TALLY["osd_x"]] == 0
    p.close()
    toy = CM.toy_dem().sector(1)                                           # a one-sector plan
    v = toy.decoder_view(0)
    p = toy.plan([L.Graph(v.indptr, v.indices, v.shape[1])], batch=BATCH)
    before = run64(L, p)
    with pytest.raises(L.QldpcError, match=r"error -1: .*two sectors"):
        p.use_correlated()
    assert np.array_equal(run64(L, p), before)
    p.close()


# ---------------------------------------------------------------------------------------- 5. the simulation entry points
def test_run_simulation_correlated(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=SEED, batch=512, **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    corr = {"alpha": 1.0, "mode": "raise"}
    r1 = run_simulation(*args, num_trials=2000, devices=[0], correlated=corr, **kw)
    r2 = run_simulation(*args, num_trials=2000, num_workers=2, devices=[0, 0], correlated=corr, **kw)
    assert r1["tally"][L.TALLY["trials"]] == 2000 and np.array_equal(r1["tally"], r2["tally"]) and r2["num_workers"] == 2
    assert r1["correlated"] == {"alpha": 1.0, "mode": "raise", "floor": None} and r1["correlated_links"] == circuit_links(L).n_links
    p = circuit_setup(L, "circ72")[6](batch=512)
    p.use_correlated(1.0, circuit_links(L))
    p.run(SEED, 0, 2000)
    assert np.array_equal(p.read(), r1["tally"])
    p.close()
    r3 = run_simulation(*args, num_trials=600, devices=[0], correlated={"mode": "condition"}, decoder="bp_osd_cs", osd_order=5, **kw)
    assert r3["decoder"] == "bp_osd_cs" and r3["correlated"]["mode"] == "condition" and r3["tally"][L.TALLY["trials"]] == 600
    r0 = run_simulation(*args, num_trials=600, devices=[0], **kw)
    assert "correlated" not in r0


def test_run_dem_simulation_correlated(L):
    from qldpc_amd.simulation.correlated import links_from_dem
    from qldpc_amd.simulation.dem import run_dem_simulation
    toy = CM.toy_dem()
    r0 = run_dem_simulation(toy, num_trials=4000, base_seed=SEED, batch=1024, devices=[0])
    r1 = run_dem_simulation(toy, num_trials=4000, base_seed=SEED, batch=1024, devices=[0], correlated={"alpha": 1.0})
    r2 = run_dem_simulation(toy, num_trials=4000, base_seed=SEED, batch=1024, devices=[0, 0], correlated={"alpha": 1.0})
    assert np.array_equal(r1["tally"], r2["tally"]) and r1["correlated_links"] == 1
    views = [toy.decoder_view(s) for s in range(2)]
    p = toy.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in views], batch=1024)
    p.use_correlated(1.0, links_from_dem(toy))
    p.run(SEED, 0, 4000)
    assert np.array_equal(p.read(), r1["tally"])
    p.close()
    T = L.TALLY
    assert r1["tally"][T["z_err"]] == r0["tally"][T["z_err"]] and r1["tally"][T["x_err"]] < r0["tally"][T["x_err"]]      # every lone A is now predicted
