"""Every handle owns its device memory, measured with the library's own count of live allocations (device_memory(): a shared card's
free-memory figure moves with other processes).  Each case builds its handles from nothing -- graphs included, since a decode grows the workspaces of
the graph it runs on -- uses them once, closes children before parents and expects (buffers, bytes) back at the reading taken before the first create.
A create or a switch that fails part-way leaves the count where it was."""
import gc
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402
import graph_shapes as GS  # noqa: E402
import window_shapes as WS  # noqa: E402
from test_relay_gpu import circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

RELAY = dict(t0=20, tr=10, max_legs=6)
DECIM = dict(alpha=0.9, t_round=10, max_rounds=6, per_round=8)
SWITCHES = {
    "plain": lambda p: None,
    "relay": lambda p: p.use_relay(**RELAY),
    "osd_cs": lambda p: p.use_osd_cs(5),
    "window": lambda p: p.use_window(4, 2),
    "layered": lambda p: p.use_layered(),
    "decimation": lambda p: p.use_decimation(**DECIM),
    "f32": lambda p: p.use_f32(),
}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def reading(L):
    gc.collect()                                  # a wrapper of an earlier test that is still waiting for the collector would free inside the bracket
    return L.device_memory()


def bb72(L):
    from qldpc_amd.data import load_code
    c = load_code("bb72")
    return c, (c["Hx_indptr"], c["Hx_indices"], int(c["n"]))


def small_case():
    return {c.name: c for c in GS.families()}["small_irregular"]


def test_the_count_follows_a_graph(L):
    c, csr = bb72(L)
    base = reading(L)
    g = L.Graph(*csr)
    made = L.device_memory()
    assert made[0] > base[0] and made[1] > base[1]
    synd = np.zeros((2, g.m), np.int8)
    synd[1, 3] = 1
    L.minsum_decode_batch(g, synd, np.full(g.n, 2.0), 5, "dynamical", 1.0)
    used = L.device_memory()
    assert used[0] > made[0] and used[1] > made[1]                       # the workspaces of the decode belong to the handle
    g.close()
    g.close()
    assert reading(L) == base


def test_code_capacity_plan_with_private_lane_graphs(L):
    c, csr = bb72(L)
    base = reading(L)
    g = L.Graph(*csr)
    per_graph = L.device_memory()[0] - base[0]
    before = L.device_memory()
    shared = L.CodeCapacityPlan(g, c["Lx"], 0.05, max_iter=10, use_osd=False, batch=64)        # fan-out lanes on the caller's graph
    n_shared = L.device_memory()[0] - before[0]
    shared.close()
    assert L.device_memory() == before
    plan = L.CodeCapacityPlan(g, c["Lx"], 0.05, max_iter=10, use_osd=True, batch=64)            # batch <= 32768 with OSD: every lane gets a graph of its own
    n_private = L.device_memory()[0] - before[0]
    assert n_private - n_shared >= 2 * per_graph, (n_private, n_shared, per_graph)             # at least two lanes hold a whole graph handle each
    plan.run(5, 0, 128)
    tally = plan.read(clear=True)
    assert tally[L.TALLY["trials"]] == 128
    plan.close()
    assert L.device_memory() == before
    g.close()
    assert reading(L) == base


def fresh_circuit(L):
    """circ72: the host side from the shared setup, graphs of its own -> (graphs, plan factory)"""
    c, compiled, M, graphs, priors, masks, _ = circuit_setup(L, "circ72")
    mine = [L.Graph(g.indptr, g.indices, g.n) for g in graphs]

    def plan(batch=16):
        return L.CircuitPlan(compiled, c["Lx"], c["Lz"], mine[0], mine[1], priors[0], priors[1], masks[0], masks[1], 0.005, batch=batch)
    return mine, plan


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_circuit_plan(L, switch):
    circuit_setup(L, "circ72")                    # (the shared setup keeps graphs of its own: made before the first reading)
    base = reading(L)
    graphs, make = fresh_circuit(L)
    p = make()
    SWITCHES[switch](p)
    p.run(3, 0, 16)
    assert p.read(clear=True)[L.TALLY["trials"]] == 16
    p.close()
    for g in graphs:
        g.close()
    assert reading(L) == base


@pytest.mark.parametrize("name", ["tiny_z", "tiny"])
def test_dem_plan_one_and_two_sectors(L, name):
    from qldpc_amd.simulation.dem import DetectorErrorModel as DEM
    dem = DM.tiny_dem(DEM)
    if name == "tiny_z":
        dem = dem.sector(0)
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    base = reading(L)
    graphs = [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views]
    p = dem.plan(graphs, max_iter=12, batch=16)
    p.run(3, 0, 16)
    assert p.read(clear=True)[L.TALLY["trials"]] == 16
    p.close()
    for g in graphs:
        g.close()
    assert reading(L) == base


def test_window_decoder(L):
    case = min(WS.families(), key=lambda c: c.m * c.n)
    W, Cm = case.configs[0]
    prior = next(iter(case.priors.values()))
    base = reading(L)
    g = L.Graph(case.indptr, case.indices, case.n)
    dec = L.WindowDecoder(g, case.layer_rows, W, Cm, prior, max_iter=10)
    assert dec.info()["graphs"] >= 1
    dec.decode(WS.syndromes(case, 2))
    dec.close()
    g.close()
    assert reading(L) == base


@pytest.mark.parametrize("kind", ["LayeredDecoder", "Minsum32Decoder"])
def test_layered_and_f32_decoders(L, kind):
    case = small_case()
    base = reading(L)
    g = L.Graph(case.indptr, case.indices, case.n)
    dec = getattr(L, kind)(g, np.full(case.n, 2.5), max_iter=10)
    err, conv, llr, iters = dec.decode(GS.syndromes(case, 2))
    assert err.shape == (2, case.n)
    dec.close()
    g.close()
    assert reading(L) == base


def test_message_stats(L):
    ip, ix = np.array([0, 1, 3, 6], np.int32), np.array([0, 0, 1, 1, 2, 3], np.int32)
    E = (np.random.default_rng(5).random((20, 4)) < 0.2).astype(np.int8)
    base = reading(L)
    g = L.Graph(ip, ix, 4)
    st = L.MessageStats(g, E, np.array([1.5, 2.5, 0.5, 3.0]), L.STATS_CHECK_MESSAGES, 0)
    st.histogram(np.linspace(-5, 5, 11))
    st.close()
    g.close()
    assert reading(L) == base


def test_comm(L):
    base = reading(L)
    comm = L.Comm.init_all(1)
    assert L.device_memory()[0] == base[0] + 1
    t = np.arange(16, dtype=np.int64)
    assert np.array_equal(comm.allreduce(t), t)
    comm.close()
    assert reading(L) == base


# ---- failure paths: ordinary error returns ------------------------------------------------------------------------------------------------------------

def test_window_create_fails_after_earlier_windows(L):
    """rows 0 | 1 | 2 as three layers, column 0 in layer 0, column 1 in layers 1 and 2: the windows at layers 0 and 1 get graphs of their own
    (different priors), the window at layer 2 has no column left"""
    g = L.Graph(np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 1], np.int32), 2)
    before = reading(L)
    with pytest.raises(L.QldpcError, match=r"error -4: the window at layer 2 has no columns"):
        L.WindowDecoder(g, 1, 1, 1, np.array([1.5, 2.5]), max_iter=5)
    assert reading(L) == before
    g.close()


def test_layered_create_fails_on_two_rows_of_a_layer_sharing_a_column(L):
    case = small_case()
    g = L.Graph(case.indptr, case.indices, case.n)
    col = int(np.flatnonzero(np.bincount(case.indices, minlength=case.n) >= 2)[0])
    a, b = [i for i in range(case.m) if col in case.indices[case.indptr[i]:case.indptr[i + 1]]][:2]
    lay = np.arange(case.m)
    lay[b] = lay[a]
    before = reading(L)
    with pytest.raises(L.QldpcError, match=f"rows {a} and {b} are both in layer"):
        L.LayeredDecoder(g, np.full(case.n, 2.5), layers=lay)
    assert reading(L) == before
    g.close()


def test_f32_create_fails_on_a_row_of_degree_57(L):
    wide = {c.name: c for c in GS.families()}["rowdeg57"]
    g = L.Graph(wide.indptr, wide.indices, wide.n)
    before = reading(L)
    with pytest.raises(L.QldpcError, match="row degree <= 56"):
        L.Minsum32Decoder(g, np.ones(wide.n))
    assert reading(L) == before
    g.close()


def test_circuit_plan_keeps_what_it_had_when_the_second_sector_fails(L):
    graphs, make = fresh_circuit(L)
    gx = graphs[1]
    col = int(np.flatnonzero(np.bincount(gx.indices, minlength=gx.n) >= 2)[0])
    a, b = [i for i in range(gx.m) if col in gx.indices[gx.indptr[i]:gx.indptr[i + 1]]][:2]
    bad = np.arange(gx.m)
    bad[b] = bad[a]
    fresh = make()
    want = fresh.run_outcomes(9, 0, 16)
    want_tally = fresh.read(clear=True)
    fresh.close()
    p = make()
    before = reading(L)
    with pytest.raises(L.QldpcError, match=f"rows {a} and {b} are both in layer"):
        p.use_layered(layers_z=np.arange(graphs[0].m), layers_x=bad)                # sector Z's decoder is built, then sector X's is refused
    assert reading(L) == before
    assert np.array_equal(p.run_outcomes(9, 0, 16), want) and np.array_equal(p.read(clear=True), want_tally)
    p.close()
    for g in graphs:
        g.close()


def test_alpha_cache_across_its_reset(L):
    c, csr = bb72(L)
    base = reading(L)
    g = L.Graph(*csr)
    synd = np.zeros((1, g.m), np.int8)
    synd[0, 5] = 1
    prior = np.full(g.n, 2.0)
    counts = []
    for k in range(70):                           # 70 schedules on one handle: the cache starts over at the 65th
        L.minsum_decode_batch(g, synd, prior, 4, "alvarado", 0.5 + k / 256.0)
        counts.append(L.device_memory()[0])
    assert counts[63] == counts[0] + 63 and counts[64] == counts[0], counts        # one device table per schedule; 64 released, one made
    g.close()
    assert reading(L) == base
