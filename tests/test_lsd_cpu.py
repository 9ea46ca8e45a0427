"""BP+LSD without a GPU: the model (tests/lsd_model.py) against the rule it restates -- flag-0 solutions reproduce the syndrome on the columns of A alone,
flags 1 and 2 arise exactly on the cases built for them, the special shots of tests/lsd_shapes.py have the properties they are named for -- the recorded
circ144 shots (every unconverged one resolves in clusters at max_rows = 512; with max_rows >= m and bits_per_step = 1 the 16 recorded OSD cases give the
reference's OSD-0 answer bit for bit), the mirror of csrc/lsd_plan.h against the header itself, and the argument rules of the Python layers."""
import os
import subprocess

import numpy as np
import pytest

import lsd_model as M
import lsd_shapes as LS
import osd_shapes as OS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default


def _residual(G, shots, b):
    return (shots.synd[b].astype(np.int64) + G.parity(shots.hard[b] & 1)) % 2


@pytest.mark.parametrize("key", sorted(LS.MATRICES))
def test_flag0_solutions_reproduce_the_syndrome(key):
    f, G = LS.matrix(key)
    shots = LS.general(key)
    for bps in (1, 2, 64):
        sol, info, traces = LS.answers(key, "general", shots, bps, 128)
        assert (info[:, 0] == 0).sum() > 12
        for b in np.flatnonzero(info[:, 0] == 0):
            assert np.array_equal(G.parity(sol[b]), shots.synd[b] & 1), (key, bps, b)
            if not _residual(G, shots, b).any():
                assert tuple(info[b]) == (0, 0, 0, 0) and np.array_equal(sol[b], shots.hard[b] & 1)
                continue
            A, piv = traces[b]["A"], traces[b]["pivots"]
            assert len(set(A)) == len(A) == info[b, 3] and set(np.flatnonzero(sol[b] != (shots.hard[b] & 1))) <= set(piv) <= set(A)
            assert info[b, 2] == LS.rows_per_round(traces[b])[-1] <= 128 and info[b, 1] == len(traces[b]["clusters"]) - 1
        assert (info[info[:, 0] != 0, 1:] == 0).all()


def test_larger_steps_take_fewer_rounds():
    shots = LS.general("ident")
    r1, r2, r64 = (LS.answers("ident", "general", shots, bps, 128)[1] for bps in (1, 2, 64))
    assert (r1[:, 0] == 0).all() and (r2[:, 0] == 0).all() and (r64[:, 0] == 0).all()          # (the identity block reaches every syndrome)
    assert (r2[:, 1] <= r1[:, 1]).all() and (r64[:, 1] <= 1).all() and r2[:, 1].sum() < r1[:, 1].sum()


def test_special_shots_are_what_they_are_named_for():
    f, G = LS.matrix("ident")
    sh = LS.single_seed()
    assert all(_residual(G, sh, b).sum() == 1 for b in range(sh.synd.shape[0]))
    info = LS.answers("ident", "single_seed", sh, 1, 128)[1]
    assert (info[:, 0] == 0).all() and (info[:, 2] == 1).any() and (info[:, 2] > 64).any()      # solved by its unit column at once / after growing over two row words
    # two seeds, one cluster after round 1
    sol, info, traces = LS.answers("dep", "merging", LS.merging(), 1, 128)
    for tr in traces:
        assert tr["clusters"][0] == [(1, 0), (1, 0)] and len(tr["clusters"][1]) == 1 and tr["clusters"][1][0][1] == 1
    # two seeds, two clusters to the end, one column each
    sol, info, traces = LS.answers("ident", "apart", LS.apart(), 1, 128)
    assert len(traces) == 6
    for b, tr in enumerate(traces):
        assert tr["clusters"] == [[(1, 0), (1, 0)], [(1, 1), (1, 1)]] and tuple(info[b]) == (0, 1, 2, 2)
    # twins: the second of a pair depends on the first
    sol, info, traces = LS.answers("doubled", "duplicates", LS.duplicates(), 2, 128)
    dependent = 0
    for b, tr in enumerate(traces):
        if info[b, 0] == 0:
            assert tr["A"][0] + 1 == tr["A"][1] and tr["A"][0] % 2 == 0 and tr["A"][1] not in tr["pivots"]      # (tied |llr|: the lower index first)
            dependent += len(tr["A"]) - len(tr["pivots"])
    assert dependent >= 5
    # seeds on rows without columns: flag 2 at every cap, also where the seeds alone pass the cap
    sh = LS.empty_rows()
    f, G = LS.matrix("tiny")
    assert sh.synd[2].sum() == 70
    for cap in (1, 64, 65, 128):
        info = LS.answers("tiny", "empty_rows", sh, 1, cap)[1]
        assert (info[:3] == [2, 0, 0, 0]).all()
        assert tuple(info[3]) == ((1, 0, 0, 0) if cap == 1 else (2, 0, 0, 0))      # (the seed WITH columns: its first column passes a cap of one row)


def test_flag1_arises_exactly_where_the_clusters_pass_the_cap():
    shots = LS.general("ident")
    free, _, traces = LS.answers("ident", "general", shots, 1, 1024)[:3]
    free_info = LS.answers("ident", "general", shots, 1, 1024)[1]
    assert (free_info[:, 0] == 0).all()
    by_one = {64: 0, 65: 0}
    for cap in (1, 64, 65):
        sol, info, _ = LS.answers("ident", "general", shots, 1, cap)
        for b in range(shots.synd.shape[0]):
            rows = LS.rows_per_round(traces[b])                              # |R| never shrinks: the cap stops the shot iff the free run ends above it
            assert info[b, 0] == (1 if free_info[b, 2] > cap else 0), (cap, b)
            if info[b, 0] == 0:
                assert np.array_equal(sol[b], free[b]) and tuple(info[b]) == tuple(free_info[b])
            elif cap in by_one and (cap, cap + 1) in zip(rows, rows[1:]):
                by_one[cap] += 1
        assert set(info[:, 0]) == {0, 1}
    assert by_one[64] >= 1 and by_one[65] >= 1                               # stopped by one row, on either side of the row-word boundary
    assert any(65 in LS.rows_per_round(tr) for tr in traces)                 # (at a cap of 65 a shot holds exactly 65 rows for a round)


def test_flagged_shots_get_osd0(oracle):
    f, G = LS.matrix("dep")
    shots = LS.general("dep")
    info = LS.answers("dep", "general", shots, 1, 64)[1]
    assert set(info[:, 0]) == {0, 1, 2}
    osd0 = lambda s, llr, hard: oracle.osd0(f.indptr, f.indices, f.n, s, llr, hard)      # noqa: E731
    for b in np.flatnonzero(info[:, 0] != 0)[:4]:
        sol, inf = M.lsd(G, shots.synd[b], shots.llr[b], shots.hard[b], 1, 64, osd0=osd0)
        assert inf == (int(info[b, 0]), 0, 0, 0) and np.array_equal(sol, osd0(shots.synd[b], shots.llr[b], shots.hard[b]))


@pytest.mark.parametrize("s", "ZX")
def test_recorded_circ144_shots(golden, s):
    """every shot of circ144_decode.npz that BP leaves unconverged ends with flag 0 at max_rows = 512; with max_rows >= m and bits_per_step = 1 the recorded
    OSD cases give the reference's OSD-0 solution bit for bit (the model's largest shot here: 299 rows, 528 columns, X 13)"""
    from qldpc_amd.data import load_circuit_matrices
    f, d = golden("circ144_decode"), load_circuit_matrices("circ144")
    G = M.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]))
    cases = [int(c) for c in f[f"{s}_osd_cases"]]
    assert len(cases) == 8 and G.m == 1008
    shot = lambda i: (f[f"{s}_syndromes"][i], f[f"{s}_llr"][i], f[f"{s}_err"][i])      # noqa: E731
    unconverged = np.flatnonzero(f[f"{s}_conv"] == 0)
    assert set(cases) <= set(unconverged)
    for i in unconverged:
        sol, info = M.lsd(G, *shot(i), 1, 512)
        assert info[0] == 0 and info[2] <= 512, (s, i, info)
        assert np.array_equal(G.parity(sol), f[f"{s}_syndromes"][i] & 1)
    for k, i in enumerate(cases):
        sol, info = M.lsd(G, *shot(i), 1, 1024)                              # (max_rows >= m = 1008: no cap at all)
        assert info[0] == 0 and info[2] <= 255 and info[3] <= 387
        assert np.array_equal(sol, f[f"{s}_osd_solution"][k]), (s, i)


def test_layout_mirror(tmp_path):
    # worked out by hand from lsd_layout for the production Z sector (1008 x 8785, columns of weight <= 6).  max_rows = 512, 8 words: U 513 * 64 = 32832,
    # 64 + 64, 4096 + 2048, lidx 2016, 2 * 1104, 6 * 1024, 512, 16, 1024 + 256 + 256, 256; max_rows = 1024, 16 words: U 1025 * 128 = 131200, 128 + 128, 8192 + 4096,
    # 2016, 2 * 1104, 6 * 2048, 1024, 16, 1536, 256
    assert LS.layout(1008, 8785, 6, 512) == 51792 and LS.layout(1008, 8785, 6, 1024) == 163088 <= LS.LDS_MAX
    assert LS.layout(1, 1, 0, 1) == 16 * 16 + 1024 + 256 + 256 + 256          # sixteen pieces of at most 16 bytes, the list and the scratch
    assert LS.supported(1008, 8785, 6, 1024) and not LS.supported(1008, 65535, 6, 1) and LS.supported(1008, 65534, 6, 512) and not LS.supported(65536, 10, 2, 1)
    assert not LS.supported(1008, 20000, 6, 1024) and LS.supported(1008, 20000, 6, 1000)      # the cap, not m, is what runs out of LDS
    assert LS.supported(65535, 300, 4, 64) and not LS.supported(65535, 300, 4, 512)          # m enters with two bytes per row
    assert LS.layout(65535, 300, 4, 64) == LS.layout(1008, 300, 4, 64) + 131072 - 2016
    exe = str(tmp_path / "lsd_layout_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "lsd_layout_main.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(OS.SEED)
    t = 20000
    m = np.concatenate([rng.integers(1, 70000, t), rng.choice([1, 64, 1008, 65535, 65536], t)])
    n = np.concatenate([rng.integers(1, 70000, t), rng.choice([1, 32, 33, 8785, 65534, 65535], t)])
    cd = rng.integers(0, 300, 2 * t)
    rows = np.concatenate([rng.integers(1, 1025, t), rng.choice([1, 63, 64, 65, 512, 960, 961, 1023, 1024], t)])
    points = [(1008, 8785, 6, 512), (1008, 8785, 6, 1024), (1, 1, 0, 1)] + list(zip(m.tolist(), n.tolist(), cd.tolist(), rows.tolist()))
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % p for p in points), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(points)
    accepted = 0
    for p, line in zip(points, out):
        lds, ok, off_misc = (int(x) for x in line.split())
        assert lds == LS.layout(*p) and off_misc == lds - 256 and bool(ok) == LS.supported(*p), (p, line)
        accepted += ok
    assert 5000 < accepted < len(points) - 5000


def test_python_argument_rules():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    from qldpc_amd.simulation import engine
    assert {"qldpc_lsd_batch", "qldpc_lsd_batch_dev", "qldpc_circuit_plan_use_lsd", "qldpc_circuit_plan_lsd_counts"} <= set(_lib.exports())
    assert _lib.lsd_params(None) == {"bits_per_step": 1, "max_rows": 512} == _lib.LSD_DEFAULTS
    assert _lib.lsd_params({"max_rows": 64}) == {"bits_per_step": 1, "max_rows": 64}
    for bad in ({"bits_per_step": 0}, {"bits_per_step": 65}, {"max_rows": 0}, {"max_rows": 1025}, {"rows": 3}, {"max_rows": 2.0}, {"bits_per_step": True}):
        with pytest.raises(ValueError):
            _lib.lsd_params(bad)
    base = dict(osd_order=0, precision="f64", decimation=None, schedule="flooding", layers=None, window=None, decoder="bp_lsd", relay_params=None, alpha_mode=None,
                alvarado_alpha=None, use_dynamic_alpha=True, scopt=False, maxIter=12, num_workers=None)
    r = engine._extension_rules(**base)
    assert r.lsd == _lib.LSD_DEFAULTS and r.path == "flooding" and not r.osd_cs
    assert engine._extension_rules(**dict(base, lsd={"bits_per_step": 4}, precision="f32")).lsd == {"bits_per_step": 4, "max_rows": 512}
    assert engine._extension_rules(**dict(base, schedule="layered")).path == "layered"
    assert engine._extension_rules(**dict(base, decoder="bp_osd")).lsd is None
    for bad in (dict(osd_order=1), dict(window=(3, 1)), dict(lsd=[1, 512]), dict(lsd={"max_rows": 2000}), dict(decoder="bp_osd", lsd={}), dict(decoder="bp_osd_cs", lsd={}),
                dict(decoder="relay_bp", lsd={}), dict(relay_params={}), dict(decoder="lsd")):
        with pytest.raises(ValueError):
            engine._extension_rules(**dict(base, **bad))

    calls = []

    class Plan:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))
    switch, _ = engine._plan_switch(engine._extension_rules(**dict(base, lsd={"max_rows": 96}, precision="f32")), [], 0)
    switch(Plan())
    assert calls == [("use_lsd", (), {"bits_per_step": 1, "max_rows": 96}), ("use_f32", (), {})]
