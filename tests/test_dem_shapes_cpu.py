"""The shape family of tests/dem_shapes.py without a GPU: every claim a case carries, the two statements of the sampler against each other, and that
the reference output of every case has something to find -- so tests/test_dem_shapes_gpu.py never compares vacuous arrays.  The decodes here are the
CPU oracle's (the checker), which the GPU decoders are held to bit for bit elsewhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402
import dem_shapes as S  # noqa: E402
import osd_shapes as OS  # noqa: E402

from qldpc_amd.simulation.dem import DetectorErrorModel  # noqa: E402

T = S.TALLY


def oracle_decode(oracle, max_iter):
    def decode(s, v, synd):
        det, conv, llr, it = oracle.minsum_decode_batch(v.indptr, v.indices, v.shape[1], synd, v.prior, max_iter=max_iter)
        return det, conv, int((it.astype(np.int64) + 1).sum()), 0
    return decode


_RUNS = {}


def oracle_run(oracle, c, max_iter=None):
    """the pipeline of a judge case on its reference sample with the oracle's min-sum and no OSD stage; once per (case, max_iter)"""
    key = (c.name, max_iter or c.max_iter)
    if key not in _RUNS:
        sampled = S.reference(c.name) if "/" not in c.name else DM.sample_sparse(c.dem, S.SEEDS[0], c.begin, c.count)
        _RUNS[key] = S.pipeline(c.dem, sampled, oracle_decode(oracle, key[1]))
    return _RUNS[key]


# ---- the two statements of the sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("name", ["tiny", "mech_1025"])
def test_sample_sparse_is_sample(name, seed):
    dem = DM.tiny_dem(DetectorErrorModel) if name == "tiny" else S.case(name).dem
    begin, count = (1 << 32) - 100, 300                          # crosses the 32-bit counter word
    want, got = DM.sample(dem, seed, begin, count), DM.sample_sparse(dem, seed, begin, count)
    for s in range(dem.n_sectors):
        for a, b in zip(got[s], want[s]):
            assert a.dtype == b.dtype == np.int8 and a.shape == b.shape and np.array_equal(a, b)
        assert want[s][0].any() and want[s][1].any()
    assert not np.array_equal(got[0][0], DM.sample_sparse(dem, seed ^ (1 << 40), begin, count)[0][0])      # the high word of the seed is read


def test_host_judge_by_hand():
    c = S.case("narrow")
    v = c.dem.decoder_view(1)                                    # columns {0, 1}, {0}, {1} with masks 1, 0, 1
    det = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1], [1, 1, 1]], np.int8)
    synd = np.array([[0, 0], [1, 1], [1, 0], [0, 0]], np.int8)
    true = np.array([[0], [0], [1], [0]], np.int8)
    err, unsat, zero = DM.judge(v, synd, det, true)
    assert err.tolist() == [False, True, False, False] and unsat.tolist() == [False, False, True, False] and zero.tolist() == [True, False, False, True]
    assert DM.predict(v, det).tolist() == [0, 1, 1, 0]
    assert not DM.judge_is_dense((4096, 4096)) and DM.judge_is_dense((40, 4097)) and DM.judge_is_dense((4097,)) and not DM.judge_is_dense((1,))
    t = np.array([[1, 0, 1], [0, 0, 0]], np.int8)
    assert DM.pack_logicals(t).tolist() == [5, 0] and np.array_equal(DM.unpack_logicals(DM.pack_logicals(t), 3), t)
    assert DM.unpack_logicals(np.zeros(4, np.uint64), 0).shape == (4, 0)


# ---- claims ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SAMPLER_CASES + S.JUDGE_CASES)
def test_claims(name):
    c = S.case(name)
    dem, counts = c.dem, S.loop_counts(c.dem)
    assert set(c.claims) <= {"mech_passes", "zero_passes", "write_passes", "word_sum", "lacc_word", "second_trials", "dense", "n", "n_mod4", "hub_degree"}
    for key in ("mech_passes", "zero_passes", "write_passes", "word_sum", "lacc_word"):
        if key in c.claims:
            assert counts[key] == c.claims[key], (name, key, counts[key])
    for s in range(dem.n_sectors):                               # what the library requires of a plan
        v = dem.decoder_view(s)
        assert v.shape[0] == dem.n_det[s] and v.prior.size == v.logmask.size == v.shape[1]
        assert dem.k[s] == 64 or not (v.logmask >> np.uint64(dem.k[s])).any()
    if c.kind == "sampler":
        assert set(c.claims) >= {"mech_passes", "zero_passes", "write_passes", "word_sum", "lacc_word"}
        return
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    assert DM.judge_is_dense(dem.n_det) == c.claims["dense"] == (name in S.DENSE_CASES)
    assert tuple(v.shape[1] for v in views) == c.claims["n"] and views[0].shape[1] % 4 == c.claims["n_mod4"]
    for s, v in enumerate(views):
        m, n = v.shape
        cdeg, rdeg = np.bincount(v.indices, minlength=n), np.diff(v.indptr)
        assert n > m and rdeg.min() >= 2, (name, s)                               # wider than tall; no row hangs on one column
        if m > 2:
            assert sorted(set(cdeg.tolist()) - {0, 1, m}) in ([2, 3], [2]) and (cdeg == m).sum() == 1, (name, s)      # degrees 2 .. 3 apart from the hub ...
            assert ((cdeg == 0) & (v.logmask != 0)).any() or dem.k[s] == 0        # ... and a column with no rows that carries a logical bit
        assert v.indices[v.indptr[m - 1]:v.indptr[m]].size >= 2                   # the last row is in use, in the view ...
        assert (dem.sectors[s].det_idx == m - 1).any()                                       # ... and in the truth
    big = views[S.big_sector(name)]
    assert np.bincount(big.indices, minlength=big.shape[1]).max() == c.claims["hub_degree"] == big.shape[0]


def test_family_covers_the_edges():
    cases = [S.case(n) for n in S.JUDGE_CASES]
    assert {c.dem.decoder_view(0).shape[1] % 4 for c in cases} >= {1, 2, 3}
    ks = [c.dem.k for c in cases]
    assert {k for pair in ks for k in pair} >= {0, 1, 64} and all(len(set(pair)) == len(pair) for pair in ks)      # k differs between the sectors
    assert S.case("narrow").dem.decoder_view(1).shape[1] == 3
    assert [S.case(n).dem.n_det for n in ("rows_4096", "rows_4097_z", "rows_4097_x", "rows_4097_one")] == [(4096, 4096), (4097, 40), (40, 4097), (4097,)]
    for c in cases:                                              # B is never a multiple of 8: the judge's last workgroup is ragged in every batch
        assert c.count % 8 and c.batch % 8 == 0 and (c.count % c.batch) % 8
    w = [S.case(n).claims["word_sum"] for n in S.SAMPLER_CASES]
    assert any(x % 2 for x in w) and any(x % 2 == 0 for x in w)  # (w0 + w1 + 1) & ~1 on odd and on even sums
    assert S.case("det_65535").dem.n_det == (65535, 1) and S.case("det_65535").dem.k == (64, 1) and S.case("one_mech").dem.k == (0,)
    assert S.case("words_256").dem.n_det == (8192,) and S.case("words_257").dem.n_det == (8193,)
    # the OSD-0 rule takes every judge matrix (tests/osd_shapes.py restates it), so each case also runs once with the OSD stage
    for c in cases:
        for s in range(c.dem.n_sectors):
            v = c.dem.decoder_view(s)
            assert not OS.rule_path(v.shape[0], v.shape[1], int(np.bincount(v.indices).max())).refused


def test_mech_4103_contents():
    c, Q = S.case("mech_4103"), S.M4103
    dem, thr = c.dem, DM.thresholds(S.case("mech_4103").dem.prob)
    assert dem.n_mech == 4103 and dem.n_mech % 4 == 3
    blocks = np.concatenate([thr, np.zeros(1, np.uint32)]).reshape(-1, 4)
    zero_blocks = sorted({l >> 2 for l in Q.zero_run})
    assert len(Q.zero_run) >= 8 and Q.zero_run[0] % 4 == 0 and not blocks[zero_blocks].any()      # whole blocks: the kernel skips them
    assert np.count_nonzero(blocks[Q.lone >> 2]) == 1 and thr[Q.lone] > 0
    assert thr[Q.thr1] == 1
    assert dem.mechanism(Q.wide, 0)[0].size >= 300
    assert dem.mechanism(Q.both, 0)[0].size and dem.mechanism(Q.both, 1)[0].size
    assert not dem.mechanism(Q.ghost, 0)[0].size and not dem.mechanism(Q.ghost, 1)[0].size and dem.mechanism(Q.ghost, 0)[1]
    crowd = [dem.mechanism(l, 0) for l in Q.crowd]
    assert len(crowd) >= 64 and all(d.size == 1 and d[0] >> 5 == Q.crowd_word and mk == 1 << Q.crowd_bit for d, mk in crowd)
    assert sum(int(d[0]) == 70 for d, _ in crowd) >= 32 and all(thr[l] == 1 << 31 for l in Q.crowd)
    lanes = {(l >> 2) % S.LANES for l in Q.crowd}
    assert len(lanes) == len(Q.crowd) and len({(l >> 2) // S.LANES for l in Q.crowd}) == 1        # one pass, a lane each
    assert len({(l >> 2) % S.LANES for l in Q.lane_mates}) == 1 and [(l >> 2) // S.LANES for l in Q.lane_mates] == [0, 1, 2, 3]
    f = DM.fires(dem.prob, S.SEEDS[0], c.begin, c.count)
    assert not f[:, list(Q.zero_run)].any() and not f[:, Q.thr1].any() and f[:, Q.lone].any() and f[:, 4102].any() and f[:, Q.ghost].any()
    n_crowd = f[:, Q.crowd].sum(axis=1)
    assert n_crowd.min() >= 16 and len(set((n_crowd % 2).tolist())) == 2                          # many of them at once, both parities


# ---- every reference has something to find -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("name", S.SAMPLER_CASES + S.JUDGE_CASES)
def test_reference_is_not_vacuous(name, seed):
    c = S.case(name)
    ref = S.reference(name, seed)
    for s, (synd, true) in enumerate(ref):
        assert synd.shape == (c.count, c.dem.n_det[s]) and true.shape == (c.count, c.dem.k[s])
        assert synd[:, -1].any() and not synd[:, -1].all(), (name, s)              # the highest detector fires in some trial, not in all
        if c.dem.k[s]:
            assert true[:, -1].any() and not true[:, -1].all(), (name, s)          # and so does bit k - 1
        assert len({r.tobytes() for r in synd}) > c.count // 4 or c.dem.n_det[s] < 8
    if hasattr(c, "last"):                                                        # the last mechanism (alone in its pass in mech_1025) fires
        assert DM.fires(c.dem.prob, seed, c.begin, c.count)[:, c.last].any()


def test_stride_second_trials_differ():
    c = S.case("stride")
    assert c.count == S.GRID + c.claims["second_trials"] and c.batch >= c.count          # one launch, min(B, 4096) workgroups
    assert c.begin < (1 << 32) < c.begin + S.GRID
    for seed in S.SEEDS:
        ref = S.reference("stride", seed)
        for s in range(2):
            synd, true = ref[s]
            late = np.arange(S.GRID, c.count)
            ds, dt = (synd[late] != synd[late - S.GRID]).any(axis=1), (true[late] != true[late - S.GRID]).any(axis=1)
            assert ds.sum() > 50 and dt.sum() > 10, (seed, s)    # a workgroup that kept its first trial's bits or accumulators would show
            stale_s, stale_t = synd[late] ^ synd[late - S.GRID], true[late] ^ true[late - S.GRID]
            assert (stale_s != synd[late]).any() and (stale_t != true[late]).any()       # (what a skipped re-zeroing would give differs too)


@pytest.mark.parametrize("name", S.JUDGE_CASES)
def test_judge_cases_reach_every_verdict(oracle, name):
    c = S.case(name)
    assert c.max_iter == 1 and S.ITERS == (1, 2)
    verdict, tally, kept = oracle_run(oracle, c, 1)              # one iteration: many BP failures
    for s in range(c.dem.n_sectors):
        x = "zx"[s]
        det, conv = kept[s]
        if c.dem.k[s]:
            assert 0 < tally[T[x + "_err"]] < c.count, (name, s, tally.tolist())          # both verdicts occur
        assert 0 < tally[T["unsat_" + x]] < c.count and 0 < tally[T["zero_synd_" + x]] < c.count, (name, s, tally.tolist())
        assert 0 < tally[T["bp_conv_" + x]] < c.count
        if det.shape[1] == 3:                                    # (narrow's second sector has no hub)
            assert det.any()
            continue
        assert det.sum(axis=1).max() > det.shape[1] // 2, (name, s)                       # a dense correction reaches the judge (the hub fired) ...
        assert (DM.judge(c.dem.decoder_view(s), S.reference(name)[s][0], det, S.reference(name)[s][1])[1] & (det.sum(axis=1) > det.shape[1] // 2)).any()      # ... unsatisfied
        assert DM.predict(c.dem.decoder_view(s), det).any() or c.dem.k[s] == 0            # the corrections carry logical action
    if name == "tail63":
        assert (kept[0][0][:, -1] == 1).all()                    # the negative prior: the last column is in every correction
    verdict2, tally2, kept2 = oracle_run(oracle, c, 2)           # two: another mix (more converge, the failures are sparse)
    assert tally2[T["bp_conv_z"]] > tally[T["bp_conv_z"]] and 0 < tally2[T["unsat_z"]] < tally[T["unsat_z"]] and not np.array_equal(kept2[0][0], kept[0][0])


@pytest.mark.parametrize("name", S.JUDGE_CASES)
def test_pointed_records(oracle, name):
    """one row set, max_iter = 1: the correction is all zeros (tail63: its last column alone), so that row alone sets the unsatisfied flag"""
    dem = S.case(name).dem
    synd, rows = S.pointed_syndromes(dem)
    assert len(rows) >= 3 * dem.n_sectors
    if name in S.DENSE_CASES:
        assert (S.big_sector(name), 4095) in rows and (S.big_sector(name), 4096) in rows
    if name == "rows_4096":
        assert (0, 4095) in rows and (1, 4095) in rows
    for s in range(dem.n_sectors):
        v = dem.decoder_view(s)
        det, conv, llr, it = oracle.minsum_decode_batch(v.indptr, v.indices, v.shape[1], synd[s], v.prior, max_iter=1)
        want = np.zeros_like(det)
        if name == "tail63":
            want[:, -1] = 1
        assert np.array_equal(det, want), (name, s, np.argwhere(det != want)[:4].tolist())
        err, unsat, zero = DM.judge(v, synd[s], det, np.zeros((det.shape[0], dem.k[s]), np.int8))
        mine = np.array([False] + [t == s for t, _ in rows])
        assert np.array_equal(unsat, mine) and np.array_equal(zero, ~mine)
        assert np.array_equal(DM.predict(v, det), np.full(det.shape[0], (1 << 63) if name == "tail63" else 0, np.uint64))


@pytest.mark.parametrize("name", S.DENSE_CASES)
def test_common_ground_decodes_alike(oracle, name):
    """with the mechanisms on row 4096 silenced, the 4097-row sector and rows_4096's sector 0 draw the same syndromes on rows 0 .. 4095 and the oracle
    corrects them alike: what the GPU test then compares between the dense and the sparse judge is the judge"""
    a, b = S.common_ground("rows_4096"), S.common_ground(name)
    sa, sb = 0, S.big_sector(name)
    ra, rb = DM.sample_sparse(a.dem, S.SEEDS[0], a.begin, a.count), DM.sample_sparse(b.dem, S.SEEDS[0], b.begin, b.count)
    assert np.array_equal(ra[sa][0], rb[sb][0][:, :4096]) and not rb[sb][0][:, 4096].any() and np.array_equal(ra[sa][1], rb[sb][1]) and ra[sa][0].any()
    na = a.dem.decoder_view(sa).shape[1]
    for max_iter in S.ITERS:
        va, ta, ka = oracle_run(oracle, a, max_iter)
        vb, tb, kb = oracle_run(oracle, b, max_iter)
        assert np.array_equal(ka[sa][0], kb[sb][0][:, :na]) and not kb[sb][0][:, na:].any() and np.array_equal(ka[sa][1], kb[sb][1])
        assert np.array_equal((va >> sa) & 1, (vb >> sb) & 1)
        for slot in S.SECTOR_SLOTS:
            assert ta[T[slot.format("zx"[sa])]] == tb[T[slot.format("zx"[sb])]], (slot, max_iter)
        assert ka[sa][0].any() and 0 < ta[T["z_err"]] < a.count and 0 < ta[T["zero_synd_z"]] < a.count and 0 < ta[T["bp_conv_z"]]
        assert ta[T["unsat_z"]] > 0 or max_iter == 2             # (two iterations correct everything that is left once the hub is silent)
