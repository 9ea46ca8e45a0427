"""Seeded detector error models at the sizes where the DEM sampler (csrc/dem.hip) and the trial judge (csrc/judge.h) change what they do, each with
the claims it was built for.  Plain module (no pytest hooks), deterministic from SEED.  tests/test_dem_shapes_cpu.py verifies every claim and that the
model's output on each case has something to find; tests/test_dem_shapes_gpu.py holds the kernels to tests/dem_model.py on them.

The arithmetic below restates the kernels' loop bounds (256 lanes, one Philox block of four mechanisms per lane, 32 detectors per LDS word, the
4096-row rule of the judge): an independent statement, not a copy the library reads."""
from types import SimpleNamespace

import numpy as np

import dem_model as DM
from qldpc_amd.simulation.dem import DecoderView, DetectorErrorModel
from qldpc_amd.simulation.engine import prior_llrs

SEED = 20261020
LANES = 256                        # threads of dem_sample_kernel
GRID = 4096                        # its largest grid: a batch beyond it gives a workgroup a second trial
HUB_PRIOR = 20.0                   # = clip_llr: a hub column's message is never one of the two smallest of a row


def _rng(name):
    return np.random.default_rng([SEED] + [ord(c) for c in name])


def _ceil(a, b):
    return (a + b - 1) // b


def loop_counts(dem):
    """passes of the three strided loops of dem_sample_kernel, the word sum its logical accumulators are placed behind, and where that puts them"""
    w = [_ceil(n, 32) for n in dem.n_det]
    return dict(mech_passes=_ceil(_ceil(dem.n_mech, 4), LANES), zero_passes=_ceil(sum(w), LANES), write_passes=_ceil(max(dem.n_det), LANES),
                word_sum=sum(w), lacc_word=(sum(w) + 1) & ~1)


# ---------------------------------------------------------------------------------------------------------------- views
def _csr_view(m, cols):
    """cols: [(rows, mask, p, prior or None)] -> DecoderView (canonical CSR over m rows, prior_llrs(p) unless a prior is given)"""
    n = len(cols)
    rows = np.concatenate([np.asarray(c[0], np.int64) for c in cols]) if n else np.zeros(0, np.int64)
    colid = np.repeat(np.arange(n, dtype=np.int64), [len(c[0]) for c in cols])
    order = np.lexsort((colid, rows))
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=indptr[1:])
    prior = np.array([prior_llrs(np.float64(c[2])) if c[3] is None else c[3] for c in cols], np.float64)
    return DecoderView(indptr.astype(np.int32), colid[order].astype(np.int32), (m, n), prior, np.array([c[1] for c in cols], np.uint64))


def _small_view(m):
    """the decoder view of a case that is only sampled: min(m, 64) chain columns (rows j and j + 1), the other rows bare"""
    n = min(m, 64)
    return _csr_view(m, [(sorted({j, (j + 1) % m}), 0, 0.01, None) for j in range(n)])


# ---------------------------------------------------------------------------------------------------------------- sampler cases
def _random_columns(rng, count, n_det, k, p, weights=(1, 2, 3)):
    """count mechanisms, each in one sector with 1 .. 3 detectors there and (three in ten) one logical bit"""
    cols = []
    for _ in range(count):
        s = int(rng.integers(len(n_det)))
        det = np.sort(rng.choice(n_det[s], min(int(rng.choice(weights)), n_det[s]), replace=False))
        mask = (1 << int(rng.integers(k[s]))) if k[s] and rng.random() < 0.3 else 0
        cols.append((float(p), [(det, mask) if t == s else ([], 0) for t in range(len(n_det))]))
    return cols


def _sampler_case(name, n_det, k, cols, count, claims, begin=(1 << 32) - 40, batch=64, **kw):
    dem = DetectorErrorModel.from_columns([c[0] for c in cols], [c[1] for c in cols], n_det, k, views=[_small_view(m) for m in n_det])
    return SimpleNamespace(name=name, kind="sampler", dem=dem, count=count, begin=begin, batch=batch, claims=claims, **kw)


def _one_mech():
    return _sampler_case("one_mech", (1,), (0,), [(0.5, [([0], 0)])], 64, dict(mech_passes=1, zero_passes=1, write_passes=1, word_sum=1, lacc_word=2))


def _mech(n_mech):
    """n_det (33, 31): words 2 + 1, an odd sum.  1024 mechanisms fill the 256 lanes once; the 1025th is alone in a second pass, and carries the highest
    detector and the highest logical bit of sector 1"""
    n_det, k = (33, 31), (5, 3)
    rng = _rng("mech_1024")                                               # (the same first 1024 mechanisms in both cases)
    cols = _random_columns(rng, 1024, n_det, k, 0.004)
    cols[3] = (0.3, [([32], 1 << 4), ([], 0)])                            # the highest detector and bit k - 1 of sector 0
    cols[1023] = (0.25, [([0, 32], 0), ([30], 1 << 2)])                   # the last word of the last lane of the first pass; both sectors
    if n_mech == 1025:
        cols.append((0.4, [([], 0), ([29, 30], 1 << 2)]))
    return _sampler_case(f"mech_{n_mech}", n_det, k, cols, 128, dict(mech_passes=1 if n_mech == 1024 else 2, zero_passes=1, write_passes=1, word_sum=3, lacc_word=4),
                         last=n_mech - 1)


M4103 = SimpleNamespace(zero_run=range(2000, 2008), lone=2010, lone_block=range(2008, 2012), thr1=5, wide=7, both=11, ghost=13, top=17,
                        crowd=[4 * b + 1 for b in range(256, 336)], crowd_word=2, crowd_bit=9, lane_mates=[4 * (40 + 256 * i) + 2 for i in range(4)])


def _mech_4103():
    """4103 mechanisms = 1026 Philox blocks: five passes of the 256 lanes, the last with two blocks, the last block ragged (three mechanisms).
    `crowd`: 80 mechanisms with p = 0.5 in consecutive blocks of the second pass -- different lanes of two waves at the same time -- that all flip
    detectors of word 2 of sector 0 (every other one the same detector, 70) and logical bit 9: the contention on one atomicXor target.  `lane_mates`:
    four mechanisms at stride-256 block positions (one lane, one per pass) on the same word and bit."""
    n_det, k, Q = (350, 40), (64, 2), M4103
    rng = _rng("mech_4103")
    cols = _random_columns(rng, 4103, n_det, k, 0.002)
    for l in Q.zero_run:
        cols[l] = (0.0, cols[l][1])                                        # blocks 500 and 501: all thresholds zero, skipped
    for l in Q.lone_block:
        cols[l] = (0.5 if l == Q.lone else 0.0, [([300 + l % 4], 1 << 20), ([], 0)])      # three dead mechanisms and a live one in one block
    cols[Q.thr1] = (2.0 ** -32, [([2], 2), ([], 0)])
    cols[Q.wide] = (0.1, [(np.arange(310), 1 << 33), ([], 0)])             # 310 detectors
    cols[Q.both] = (0.2, [([5, 349], 1 << 7), ([1, 39], 2)])               # both sectors, the highest detector of each, bit k - 1 of sector 1
    cols[Q.ghost] = (0.1, [([], 1 << 62), ([], 0)])                         # an undetectable logical flip
    cols[Q.top] = (0.15, [([349], 1 << 63), ([], 0)])
    for i, l in enumerate(Q.crowd):
        cols[l] = (0.5, [([70 if i % 2 else 64 + (i // 2) % 32], 1 << Q.crowd_bit), ([], 0)])
    for l in Q.lane_mates:
        cols[l] = (0.5, [([70], 1 << Q.crowd_bit), ([], 0)])
    cols[4102] = (0.3, [([348], 0), ([38], 1)])                            # the last mechanism of the ragged last block
    return _sampler_case("mech_4103", n_det, k, cols, 128, dict(mech_passes=5, zero_passes=1, write_passes=2, word_sum=13, lacc_word=14), marks=Q)


def _words(n_det):
    """one sector of 8192 / 8193 detectors: 256 / 257 words, so the zeroing loop ends after one pass / needs lane 0 a second time; the write-out loop
    takes 32 / 33 passes.  The highest detector is flipped by mechanism 0."""
    rng = _rng(f"words_{n_det}")
    cols = _random_columns(rng, 600, (n_det,), (3,), 0.01)
    cols[0] = (0.3, [([n_det - 2, n_det - 1], 1 << 2)])
    w = _ceil(n_det, 32)
    return _sampler_case(f"words_{w}", (n_det,), (3,), cols, 64, dict(mech_passes=1, zero_passes=_ceil(w, 256), write_passes=_ceil(n_det, 256), word_sum=w,
                                                                       lacc_word=(w + 1) & ~1))


def _det_65535():
    """the LDS maximum: sectors of 65535 and 1 detectors (2048 + 1 words: an odd sum, the accumulators behind word 2050), k = (64, 1)"""
    n_det, k = (65535, 1), (64, 1)
    rng = _rng("det_65535")
    cols = _random_columns(rng, 500, n_det, k, 0.02)
    cols[0] = (0.3, [([65534], 1 << 63), ([], 0)])
    cols[1] = (0.3, [([0, 65533], 0), ([0], 1)])
    return _sampler_case("det_65535", n_det, k, cols, 64, dict(mech_passes=1, zero_passes=9, write_passes=256, word_sum=2049, lacc_word=2050))


def _stride():
    """mech_1025's model at batch 8192: one launch of 4096 workgroups for 4196 trials, so workgroups 0 .. 99 take trials t and t + 4096"""
    c = _mech(1025)
    return SimpleNamespace(name="stride", kind="sampler", dem=c.dem, count=GRID + 100, begin=(1 << 32) - 4000, batch=2 * GRID, last=c.last,
                           claims=dict(c.claims, second_trials=100))


# ---------------------------------------------------------------------------------------------------------------- judge cases
A_ROWS, A_EXTRA = 4096, 301
A_N = A_ROWS + A_EXTRA + 4          # mechanisms of a big block: chain, extra, bare, hub, two that touch row 4096 alone
A_BARE, A_HUB, A_ISO = A_ROWS + A_EXTRA, A_ROWS + A_EXTRA + 1, (A_ROWS + A_EXTRA + 2, A_ROWS + A_EXTRA + 3)


def _masks(rng, n, k):
    """a logical mask on every fourth column (k = 64: random words; k = 1: bit 0)"""
    out = [0] * n
    for j in range(0, n, 4):
        out[j] = int(rng.integers(1, 1 << 63)) | (int(rng.integers(2)) << 63) if k == 64 else ((1 << int(rng.integers(k))) if k else 0)
    return out


def _tilt(p, j, chain):
    """the probability of column j: the chain's even columns are likelier than its odd ones, so that when the hub fires (every row unsatisfied) one
    iteration already flips the even half of the chain -- a dense correction that does not reproduce the syndrome"""
    return p * (1.3 if j % 2 == 0 else 0.7) if j < chain else p


def _big_block(name, k):
    """columns over rows 0 .. 4096, the same whichever sector height takes them: a chain over rows 0 .. 4095 (column j = rows j, j + 1 mod 4096: degree 2),
    301 columns of degree 3, a bare column with a logical bit, the hub (every row; prior HUB_PRIOR) and two columns on row 4096 alone.  A sector of
    4096 rows drops row 4096: the last two become empty mechanisms and leave its view."""
    rng = _rng(name)
    rows = [[j, (j + 1) % A_ROWS] for j in range(A_ROWS)] + [sorted(rng.choice(A_ROWS, 3, replace=False).tolist()) for _ in range(A_EXTRA)]
    masks = _masks(rng, len(rows), k)
    if k == 64:
        masks[A_ROWS - 1] |= 1 << 63                                        # the column of rows 4095 and 0
    p = 1.6 / len(rows)                                                     # one trial in five has no firing mechanism among these
    cols = [(r, mk, _tilt(p, j, A_ROWS), None) for j, (r, mk) in enumerate(zip(rows, masks))]
    top = (1 << (k - 1)) if k else 0
    cols.append(([], top | (1 if k else 0), 0.2, None))                      # bare: no rows, a logical bit
    cols.append((list(range(A_ROWS + 1)), (1 << 5) if k == 64 else 0, 0.05, HUB_PRIOR))
    cols += [([A_ROWS], top, 0.1, None), ([A_ROWS], 0, 0.1, None)]
    assert len(cols) == A_N
    return cols


def _small_block(name, m, extra, k, hub=True):
    """the same make at m rows: chain, `extra` columns of degree 3, a bare column, the hub"""
    rng = _rng(name)
    rows = [sorted({j, (j + 1) % m}) for j in range(m)] + [sorted(rng.choice(m, 3, replace=False).tolist()) for _ in range(extra)]
    masks = _masks(rng, len(rows), k)
    p = 1.6 / len(rows)
    cols = [(r, mk, _tilt(p, j, m), None) for j, (r, mk) in enumerate(zip(rows, masks))]
    top = (1 << (k - 1)) if k else 0
    cols.append(([], top, 0.2, None))
    if hub:
        cols.append((list(range(m)), top, 0.05, HUB_PRIOR))
    return cols


def _judge_case(name, blocks, n_det, k, claims, cross=(), count=77, batch=48, max_iter=1, view_extra=None):
    """blocks[s]: the columns of sector s; the mechanisms are sector 0's columns, then sector 1's, each touching its own sector, then `cross`
    ((p, [(rows, mask) per sector]): mechanisms in both).  The view of a sector is its columns with the rows the sector has, without those left empty
    and without a logical bit by the cut; view_extra[s]: view-only columns appended."""
    nsec = len(n_det)
    prob, columns, views, first = [], [], [], [0]
    for s, cols in enumerate(blocks):
        kept = []
        for rows, mask, p, prior in cols:
            cut = [r for r in rows if r < n_det[s]]
            dead = bool(rows) and not cut                                   # touched only rows this sector does not have
            prob.append(p)
            columns.append([(cut, 0 if dead else mask) if t == s else ([], 0) for t in range(nsec)])
            if not dead:
                kept.append((cut, mask, p, prior))
        views.append(_csr_view(n_det[s], kept + list((view_extra or {}).get(s, []))))
        first.append(len(prob))
    for p, proj in cross:
        prob.append(p)
        columns.append(list(proj))
    dem = DetectorErrorModel.from_columns(prob, columns, n_det, k, views=views)
    return SimpleNamespace(name=name, kind="judge", dem=dem, count=count, batch=batch, begin=1000, max_iter=max_iter, first=first, claims=claims)


def _rows_4096():
    return _judge_case("rows_4096", [_big_block("A64", 64), _big_block("A1", 1)], (4096, 4096), (64, 1),
                       dict(dense=False, n=(A_N - 2, A_N - 2), n_mod4=3, hub_degree=4096))


def _rows_4097_z():
    return _judge_case("rows_4097_z", [_big_block("A64", 64), _small_block("S0", 40, 8, 0)], (4097, 40), (64, 0),
                       dict(dense=True, n=(A_N, 50), n_mod4=1, hub_degree=4097))


def _rows_4097_x():
    # the big block comes first among the mechanisms although it is sector 1's: it keeps the mechanism numbers it has in rows_4096
    c = _judge_case("rows_4097_x", [_big_block("A64", 64), _small_block("S1", 40, 9, 1)], (4097, 40), (64, 1), dict())
    d = c.dem
    swapped = DetectorErrorModel(d.prob, [tuple(d.sectors[1]), tuple(d.sectors[0])], [d.decoder_view(1), d.decoder_view(0)])
    return SimpleNamespace(name="rows_4097_x", kind="judge", dem=swapped, count=77, batch=48, begin=1000, max_iter=1, first=c.first,
                           claims=dict(dense=True, n=(51, A_N), n_mod4=3, hub_degree=4097))


def _rows_4097_one():
    return _judge_case("rows_4097_one", [_big_block("A64", 64)], (4097,), (64,), dict(dense=True, n=(A_N,), n_mod4=1, hub_degree=4097))


def _narrow():
    """sector 1's view has three columns over two rows; sector 0 has 70 rows and 82 columns (n % 4 = 2); one mechanism hits both sectors"""
    s1 = [([0, 1], 1, 0.3, None), ([0], 0, 0.1, None), ([1], 1, 0.2, None)]
    return _judge_case("narrow", [_small_block("N0", 70, 10, 3), s1], (70, 2), (3, 1), dict(dense=False, n=(82, 3), n_mod4=2, hub_degree=70),
                       cross=[(0.1, [([3, 69], 1 << 2), ([1], 1)])], count=203, batch=64)


def _tail63():
    """one sector, 37 rows, k = 64, n = 49 (n % 4 = 1); the view's last column has a negative prior, no rows and logical bit 63: every correction has
    det[n - 1] = 1, and for the shots whose correction starts dword-aligned that column is the one tail byte of the judge's scan"""
    last = [([], 1 << 63, 0.88, None)]
    c = _judge_case("tail63", [_small_block("T0", 37, 9, 64)], (37,), (64,), dict(dense=False, n=(49,), n_mod4=1, hub_degree=37),
                    count=203, batch=64, view_extra={0: last})
    return c


BUILDERS = {"one_mech": _one_mech, "mech_1024": lambda: _mech(1024), "mech_1025": lambda: _mech(1025), "mech_4103": _mech_4103,
            "words_256": lambda: _words(8192), "words_257": lambda: _words(8193), "det_65535": _det_65535, "stride": _stride,
            "rows_4096": _rows_4096, "rows_4097_z": _rows_4097_z, "rows_4097_x": _rows_4097_x, "rows_4097_one": _rows_4097_one, "narrow": _narrow,
            "tail63": _tail63}
SAMPLER_CASES = ("one_mech", "mech_1024", "mech_1025", "mech_4103", "words_256", "words_257", "det_65535", "stride")
JUDGE_CASES = ("rows_4096", "rows_4097_z", "rows_4097_x", "rows_4097_one", "narrow", "tail63")
DENSE_CASES = ("rows_4097_z", "rows_4097_x", "rows_4097_one")
ITERS = (1, 2)                                                               # max_iter of the plans: BP failures reach the judge
SEEDS = (20260301, (0x9E3779B9 << 32) | 17)                                  # the second has a non-zero high word
_CASES, _REFS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def reference(name, seed=SEEDS[0]):
    """DM.sample_sparse of a case on its own range: computed once per (case, seed), shared by the tests and left unchanged"""
    if (name, seed) not in _REFS:
        c = case(name)
        ref = DM.sample_sparse(c.dem, seed, c.begin, c.count)
        for a, b in ref:
            a.setflags(write=False)
            b.setflags(write=False)
        _REFS[(name, seed)] = ref
    return _REFS[(name, seed)]


def big_sector(name):
    """the sector of a judge case that holds the big block"""
    return 1 if name == "rows_4097_x" else 0


def common_ground(name):
    """The case with every mechanism that touches row 4096 silenced (the hub and the two on row 4096 alone; in rows_4096 the same mechanism numbers,
    so the draws of all others stay where they are).  What is left draws and decodes alike at 4096 and 4097 rows: the hub's message has magnitude
    >= HUB_PRIOR = clip_llr, above every other prior, so it is never one of a row's two smallest and its sign stays positive while only a few rows
    are unsatisfied; row 4096 then talks to nobody but the hub and its own two columns."""
    c = case(name)
    prob = c.dem.prob.copy()
    prob[[A_HUB, *A_ISO]] = 0.0
    dem = DetectorErrorModel(prob, [tuple(S) for S in c.dem.sectors], [c.dem.decoder_view(s) for s in range(c.dem.n_sectors)])
    return SimpleNamespace(name=name + "/common", kind="judge", dem=dem, count=c.count, batch=c.batch, begin=c.begin, max_iter=c.max_iter, first=c.first, claims=c.claims)


def pointed_rows(m):
    """the rows a pointed record sets, one per record: 0, 31, 32, m - 1 and, where they exist, 4095 and 4096"""
    return sorted({r for r in (0, 31, 32, m - 1, 4095, 4096) if 0 <= r < m})


def pointed_syndromes(dem):
    """per sector int8[R, m]: the empty record first, then one record per pointed row of sector 0, then of sector 1 (the other sector stays empty)"""
    rows = [(s, r) for s in range(dem.n_sectors) for r in pointed_rows(dem.n_det[s])]
    out = [np.zeros((1 + len(rows), m), np.int8) for m in dem.n_det]
    for i, (s, r) in enumerate(rows):
        out[s][1 + i, r] = 1
    return out, rows


# ---------------------------------------------------------------------------------------------------------------- the pipeline in parts
TALLY = {"trials": 0, "z_err": 1, "x_err": 2, "total_err": 3, "bp_conv_z": 4, "bp_conv_x": 5, "osd_z": 6, "osd_x": 7, "iters_z": 8, "iters_x": 9,
         "zero_synd_z": 10, "zero_synd_x": 11, "unsat_z": 12, "unsat_x": 13, "legs_z": 14, "legs_x": 15}      # include/qldpc_hip.h, QLDPC_TALLY_*
SECTOR_SLOTS = ("{}_err", "bp_conv_{}", "osd_{}", "iters_{}", "zero_synd_{}", "unsat_{}")      # the slots one sector owns ({} = z or x)


def pipeline(dem, sampled, decode):
    """sampled: [(syndromes, true) per sector]; decode(sector, view, syndromes) -> (det, conv, iterations summed, osd calls).  The host judge on every
    sector -> (verdicts uint8[count] with bit s = logical error of sector s, the 16 tally slots, [(det, conv) per sector])"""
    count = sampled[0][0].shape[0]
    tally, verdict, kept = np.zeros(16, np.int64), np.zeros(count, np.uint8), []
    tally[TALLY["trials"]] = count
    for s in range(dem.n_sectors):
        v, (synd, true) = dem.decoder_view(s), sampled[s]
        det, conv, iters, osd = decode(s, v, synd)
        err, unsat, zero = DM.judge(v, synd, det, true)
        verdict |= err.astype(np.uint8) << s
        x = "zx"[s]
        tally[TALLY[x + "_err"]], tally[TALLY["bp_conv_" + x]], tally[TALLY["osd_" + x]], tally[TALLY["iters_" + x]] = err.sum(), (conv != 0).sum(), osd, iters
        tally[TALLY["zero_synd_" + x]], tally[TALLY["unsat_" + x]] = zero.sum(), unsat.sum()
        kept.append((det, conv))
    tally[TALLY["total_err"]] = np.count_nonzero(verdict)
    return verdict, tally, kept

