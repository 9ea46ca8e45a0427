"""Recorded detection events on the MI355X: the unpacker against the numpy model bit for bit (E1), events in and the plan's own verdicts out (E2), every
decoder switch against the batch decoder it stands for (E3), a decode as a function of (record, seed, shot index) (E4), arguments (E5) and the Python
surface (E6).  Every shot of every test is compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402
import events_model as EM  # noqa: E402

pytestmark = pytest.mark.gpu

RELAY = dict(t0=20, tr=10, max_legs=6)
DECIM = dict(alpha=0.9, t_round=10, max_rounds=6, per_round=8)
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def DEM():
    from qldpc_amd.simulation.dem import DetectorErrorModel
    return DetectorErrorModel


_MODELS = {}


def model(L, DEM, name):
    """(dem, graphs) of "tiny", "circ72" (layer_rows 36) and their sector-0 halves "tiny_z", "circ72_z"; built once."""
    if name not in _MODELS:
        if name.endswith("_z"):
            dem = model(L, DEM, name[:-2])[0].sector(0)
        else:
            dem = DM.tiny_dem(DEM) if name == "tiny" else DEM.from_decoding_matrices("circ72", layer_rows=36)
        views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
        _MODELS[name] = (dem, [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views])
    return _MODELS[name]


def default_records(syndromes):
    """the sectors' syndromes as records in the default layout (sector 0's rows, then sector 1's)"""
    n_bits, tabs = EM.default_layout([s.shape[1] for s in syndromes])
    return EM.embed(syndromes, n_bits, tabs)


def verdicts(pred, truth):
    """bit s = the prediction of sector s differs from the truth in some observable"""
    out = np.zeros(truth[0].shape[0], np.uint8)
    for s, t in enumerate(truth):
        out |= (EM.pred_bits(pred[s], t.shape[1]) != t).any(axis=1).astype(np.uint8) << np.uint8(s)
    return out


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, f"{what}: shots {bad[:8].tolist()} differ ({bad.size} of {got.shape[0]}): got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}"
    return True


# ---- E1 -----------------------------------------------------------------------------------------------------------------------------------------------
def interleaved_layout():
    """n_bits = 61 on tiny (37 + 5 rows): the sectors alternate on bits 0..9, the rest of sector 0 runs DOWN from bit 60; three rows are -1, rows 20 and
    21 of sector 0 name one bit, and bits 10..28 and 40 are named by no row."""
    t0 = np.concatenate([2 * np.arange(5), 60 - np.arange(32)]).astype(np.int32)
    t1 = (2 * np.arange(5) + 1).astype(np.int32)
    t0[10] = t0[36] = t1[2] = -1
    t0[21] = t0[20]
    named = set(t0[t0 >= 0].tolist()) | set(t1[t1 >= 0].tolist())
    assert len(named) == 37 + 5 - 3 - 1 and not named & set(range(10, 29)) and max(named) == 60
    return 61, [t0, t1]


@pytest.mark.parametrize("stride", [8, 11])
@pytest.mark.parametrize("layout", ["default", "interleaved"])
def test_e1_unpacker_is_the_model_tiny(L, DEM, layout, stride):
    dem, graphs = model(L, DEM, "tiny")
    count = 1027                                                # four full batches and a ragged fifth
    n_bits, tabs = EM.default_layout(dem.n_det) if layout == "default" else interleaved_layout()
    rng = np.random.default_rng(1000 * stride + len(layout))
    bits = np.ones((count, 8 * stride), np.uint8)               # every padding byte and the unused high bits of the last byte are ones
    bits[:, :n_bits] = rng.random((count, n_bits)) < 0.5        # density 0.5: a wrong bit cannot hide
    records = EM.pack(bits)
    assert records.shape == (count, stride) and (records[:, (n_bits + 7) // 8:] == 0xFF).all() and (records[:, (n_bits - 1) >> 3] >> (n_bits % 8 or 8) == (0xFF >> (n_bits % 8 or 8))).all()
    want = EM.gather(records, n_bits, tabs)
    plan = dem.plan(graphs, batch=256)
    if layout != "default":
        plan.set_event_layout(n_bits, *tabs)
    got = plan.unpack_events(records)
    plan.close()
    for s in range(2):
        assert got[s].dtype == np.int8
        assert_same(got[s], want[s], f"sector {s}")
    assert all(0.4 < w.mean() < 0.6 for w in (want[0][:, :10], want[1][:, [0, 1, 3, 4]]))


def test_e1_unpacker_is_the_model_circ72(L, DEM):
    dem, graphs = model(L, DEM, "circ72")
    count, (n_bits, tabs) = 300, EM.default_layout(dem.n_det)
    assert dem.n_det[0] % 4 == 0 and n_bits == 576
    records = EM.pack(np.random.default_rng(72).random((count, n_bits)) < 0.5)
    want = EM.gather(records, n_bits, tabs)
    plan = dem.plan(graphs, batch=128)
    got = plan.unpack_events(records)
    for s in range(2):
        assert_same(got[s], want[s], f"sector {s}")
    # an odd stride moves every record's address: its first byte sits at every offset inside a dword
    odd = np.hstack([records, np.full((count, 3), 0xFF, np.uint8)])
    got = plan.unpack_events(odd)
    plan.close()
    for s in range(2):
        assert_same(got[s], want[s], f"stride 75, sector {s}")
    # the sector-0 half alone: 288 rows per shot, the table-free run at base 0 of a 288-bit record
    z, zg = model(L, DEM, "circ72_z")
    zp = z.plan(zg, batch=128)
    gz = zp.unpack_events(records[:, :36])
    zp.close()
    assert assert_same(gz[0], want[0], "one sector") and gz[1].size == 0


def test_e1_rows_beyond_one_pass_and_unaligned_row_base(L, DEM):
    """The shipped circ288 model has 2880 rows per sector: more than the 1024 rows a 256-lane workgroup writes in one pass.  A table that drops into the
    middle of the default run exercises the gather on the same shape, and tiny's 37 + 5 rows per shot (above) give every alignment of a shot's row base."""
    dem = DEM.from_decoding_matrices("circ288")
    views = [dem.decoder_view(s) for s in range(2)]
    graphs = [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views]
    count, (n_bits, tabs) = 40, EM.default_layout(dem.n_det)
    assert dem.n_det[0] > 1024
    records = EM.pack(np.random.default_rng(288).random((count, n_bits)) < 0.5)
    plan = dem.plan(graphs, batch=16)
    got = plan.unpack_events(records)
    want = EM.gather(records, n_bits, tabs)
    for s in range(2):
        assert_same(got[s], want[s], f"default, sector {s}")
    tabs[1] = tabs[1][::-1].copy()                              # sector 1 reads its run backwards: a table; sector 0 keeps the run
    tabs[1][1500] = -1
    plan.set_event_layout(n_bits, None, tabs[1])
    got = plan.unpack_events(records)
    plan.close()
    want = EM.gather(records, n_bits, tabs)
    for s in range(2):
        assert_same(got[s], want[s], f"reversed, sector {s}")


# ---- E2 -----------------------------------------------------------------------------------------------------------------------------------------------
def plain_corrections(L, dem, graphs, syndromes, max_iter):
    """per sector (det, conv) of the batch decoders a fresh plan stands for: min-sum, then OSD-0 on the non-converged"""
    out = []
    for s in range(dem.n_sectors):
        g, v, synd = graphs[s], dem.decoder_view(s), syndromes[s]
        det, conv, llr, _ = L.minsum_decode_batch(g, synd, v.prior, max_iter, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        if bad.size:
            det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
        out.append((det, conv))
    return out


def check_against_run(L, dem, graphs, plan, seed, begin, count, corrections=None):
    """E2's identities for one range on `plan`; corrections(syndromes) -> [(det, conv) per sector] of the batch decoders, which then pin pred and the
    flags without the plan's judge.  Returns (records, pred0, pred1, flags)."""
    T, ns = L.TALLY, dem.n_sectors
    sampled = plan.sample(seed, begin, count)
    synd, truth = [sampled[2 * s] for s in range(ns)], [sampled[2 * s + 1] for s in range(ns)]
    outcome = plan.run_outcomes(seed, begin, count)
    tally = plan.read(clear=True)
    records = default_records(synd)
    before = plan.read()
    pred0, pred1, flags = plan.decode_events(records, seed, begin)
    assert np.array_equal(plan.read(), before) and not before.any()      # the tally is not touched
    pred = (pred0, pred1)
    assert_same(verdicts(pred, truth), outcome, "verdicts")
    for s in range(ns):
        assert int(((flags >> s) & 1).sum()) == tally[T["bp_conv_" + "zx"[s]]], f"sector {s}: converged flags against the tally"
        assert_same((flags >> (4 + s)) & 1, ~synd[s].any(axis=1), f"sector {s}: zero-syndrome flag")
        assert int(((flags >> (2 + s)) & 1).sum()) == tally[T["unsat_" + "zx"[s]]]
    if ns == 1:
        assert not pred1.any() and not (flags & 0x2A).any()
    if corrections is not None:
        for s, (det, conv) in enumerate(corrections(synd)):
            assert_same(pred[s], EM.predict(det, dem.decoder_view(s).logmask), f"sector {s}: prediction against the batch decoder's correction")
            assert_same((flags >> s) & 1, conv != 0, f"sector {s}: converged flag")
            assert_same((flags >> (2 + s)) & 1, (L.gf2_spmv_batch(graphs[s], det) != (synd[s] & 1)).any(axis=1), f"sector {s}: unsatisfied flag")
    return records, pred0, pred1, flags


@pytest.mark.parametrize("name, count, batch, seed, begin", [("tiny", 4096, 1024, 424242, 0), ("tiny", 4096, 1024, (0x9E3779B9 << 32) | 17, 2 ** 32 - 100),
                                                             ("circ72", 512, 128, 424242, 0), ("tiny_z", 4096, 1024, 424242, 0), ("circ72_z", 512, 128, 424242, 0)])
def test_e2_events_in_verdicts_out(L, DEM, name, count, batch, seed, begin):
    dem, graphs = model(L, DEM, name)
    plan = dem.plan(graphs, max_iter=12, batch=batch)
    _, pred0, pred1, flags = check_against_run(L, dem, graphs, plan, seed, begin, count, lambda synd: plain_corrections(L, dem, graphs, synd, 12))
    plan.close()
    assert pred0.any() and (flags & 1).any() and not (flags & 1).all() or name.startswith("tiny")      # BP failures on circ72: the OSD stage had work
    if name == "tiny":
        assert (pred0 >> np.uint64(63)).any() and pred1.any()   # bit 63 and sector 1 are exercised


# ---- E3 -----------------------------------------------------------------------------------------------------------------------------------------------
def _switches(L, seed, begin, max_iter):
    """per switch (use(plan), decode(sector, graph, view, syndromes) -> (det, conv)): the batch decoder every plan switch stands for"""
    from qldpc_amd.decoding.decimation import DecimationDecoder
    from qldpc_amd.decoding.layered import LayeredMinSumDecoder
    from qldpc_amd.decoding.single import SingleMinSumDecoder
    from qldpc_amd.decoding.window import SlidingWindowDecoder
    H = lambda g: (g.indptr, g.indices, g.n)      # noqa: E731

    def then_osd(bp, cs_order=None):
        def decode(s, g, v, synd):
            det, conv, llr = bp(s, g, v, synd)
            det = det.copy()
            bad = np.flatnonzero(conv == 0)
            if bad.size:
                det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad]) if cs_order is None else L.osdcs_batch(g, synd[bad], llr[bad], det[bad], v.prior, cs_order)[0]
            return det, conv
        return decode

    def minsum(s, g, v, synd):
        return L.minsum_decode_batch(g, synd, v.prior, max_iter, "dynamical", 1.0)[:3]

    def relay(s, g, v, synd):                     # the call's seed, the global shot index as the shot, the sector as the tag; no OSD stage
        return L.relay_decode_batch(g, synd, v.prior, seed, begin, s, **RELAY)[:2]

    def layered(s, g, v, synd):
        return LayeredMinSumDecoder(H(g), v.prior, maxIter=max_iter).decode(synd)[:3]

    def decim(s, g, v, synd):
        det, llr, conv = DecimationDecoder(H(g), v.prior, clip_llr=20.0, **DECIM).decode(synd)[:3]
        return det, conv, llr

    def single(s, g, v, synd):
        return SingleMinSumDecoder(H(g), v.prior, max_iter=max_iter).decode(synd)[:3]

    def window(s, g, v, synd):
        err, info = SlidingWindowDecoder(H(g), v.prior, 36, 3, 1, max_iter=max_iter).decode(synd)
        return err, (info["conv"] == info["windows"]).astype(np.uint8)

    return {"relay": (lambda p: p.use_relay(**RELAY), relay),
            "osd_cs": (lambda p: p.use_osd_cs(4), then_osd(minsum, cs_order=4)),
            "layered": (lambda p: p.use_layered(), then_osd(layered)),
            "decimation": (lambda p: p.use_decimation(**DECIM), then_osd(decim)),
            "f32": (lambda p: p.use_f32(), then_osd(single)),
            "window": (lambda p: p.use_window(3, 1), window)}


@pytest.mark.parametrize("name", ["circ72", "circ72_z"])
@pytest.mark.parametrize("switch", ["relay", "osd_cs", "layered", "decimation", "f32", "window"])
def test_e3_switches_ride_along(L, DEM, name, switch):
    dem, graphs = model(L, DEM, name)
    seed, begin, count, max_iter = 777, 1000, 128, 12
    use, decode = _switches(L, seed, begin, max_iter)[switch]
    plan = dem.plan(graphs, max_iter=max_iter, batch=128)
    use(plan)
    check_against_run(L, dem, graphs, plan, seed, begin, count,
                      lambda synd: [decode(s, graphs[s], dem.decoder_view(s), synd[s]) for s in range(dem.n_sectors)])
    plan.close()


# ---- E4 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, relay", [("circ72", True), ("tiny", False)])
def test_e4_function_of_record_seed_and_shot_index(L, DEM, name, relay):
    dem, graphs = model(L, DEM, name)
    seed, begin, count = 31337, 5000, 384

    def make(batch):
        p = dem.plan(graphs, max_iter=12, batch=batch)
        if relay:
            p.use_relay(**RELAY)
        return p

    plan = make(128)
    sampled = plan.sample(seed, begin, count)
    records = default_records([sampled[0], sampled[2]])
    fresh = plan.run_outcomes(seed, begin, count)
    fresh_tally = plan.read(clear=True)
    before = plan.read()
    one = plan.decode_events(records, seed, begin)
    assert np.array_equal(plan.read(), before)                  # plan.read() is what it was
    assert_same(verdicts(one[:2], [sampled[1], sampled[3]]), fresh, "verdicts")
    # three calls of 128 with shot_begin advanced
    parts = [plan.decode_events(records[i:i + 128], seed, begin + i) for i in range(0, count, 128)]
    for k, what in enumerate(("pred0", "pred1", "flags")):
        assert_same(np.concatenate([p[k] for p in parts]), one[k], f"three calls: {what}")
    # a run after the decodes returns what it returns on a fresh plan: no counter or buffer leaks
    assert_same(plan.run_outcomes(seed, begin, count), fresh, "run_outcomes after decode_events")
    assert np.array_equal(plan.read(clear=True), fresh_tally)
    # another batch size
    small = make(64)
    for k, what in enumerate(("pred0", "pred1", "flags")):
        assert_same(small.decode_events(records, seed, begin)[k], one[k], f"batch 64: {what}")
    small.close()
    # the _dev form on torch tensors, then a stream sync
    dev = torch.device("cuda", 0)
    d_rec = torch.from_numpy(records).to(dev)
    d_p0, d_p1 = torch.full((count,), -1, dtype=torch.int64, device=dev), torch.full((count,), -1, dtype=torch.int64, device=dev)
    d_fl = torch.full((count,), 0xFF, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    plan.decode_events_dev(d_rec.data_ptr(), count, records.shape[1], d_p0.data_ptr(), d_p1.data_ptr(), d_fl.data_ptr(), seed=seed, shot_begin=begin,
                           stream=stream.cuda_stream)
    stream.synchronize()
    assert_same(d_p0.cpu().numpy().view(np.uint64), one[0], "_dev: pred0")
    assert_same(d_p1.cpu().numpy().view(np.uint64), one[1], "_dev: pred1")
    assert_same(d_fl.cpu().numpy(), one[2], "_dev: flags")
    if relay:                                                   # the shot index matters to Relay-BP and to nothing else: the test would not see a dropped offset otherwise
        moved = plan.decode_events(records, seed, begin + 1)
        assert (moved[2] != one[2]).any() or (moved[0] != one[0]).any() or (moved[1] != one[1]).any()
    plan.close()


# ---- E5 -----------------------------------------------------------------------------------------------------------------------------------------------
def _err(L):
    return (L.lib().qldpc_last_error() or b"").decode()


def test_e5_arguments(L, DEM):
    dem, graphs = model(L, DEM, "tiny")
    plan = dem.plan(graphs, max_iter=12, batch=64)
    lib, h = L.lib(), plan._h
    count = 8
    rec = np.zeros((count, 6), np.uint8)
    p0, p1, fl = np.full(count, 7, np.uint64), np.full(count, 7, np.uint64), np.full(count, 7, np.uint8)
    u8, u64 = (lambda a: L.ptr(a, C.c_uint8)), (lambda a: L.ptr(a, C.c_uint64))

    def decode(plan_h=h, n=count, begin=0, events=rec, stride=6, a=p0, b=p1, f=fl, fn=lib.qldpc_circuit_plan_decode_events):
        opt = lambda x, conv: conv(x) if x is not None else None      # noqa: E731
        return fn(plan_h, 5, begin, n, opt(events, u8), stride, None, opt(a, u64), opt(b, u64), opt(f, u8))

    for kw, needle in [(dict(plan_h=None), "plan"), (dict(events=None), "events"), (dict(a=None), "pred0"), (dict(b=None), "pred1"), (dict(f=None), "flags"),
                       (dict(n=-1), "count"), (dict(begin=-1), "shot_begin"), (dict(stride=5), "stride")]:
        assert decode(**kw) == INVALID and needle in _err(L), (kw, _err(L))
    dev_fn = lib.qldpc_circuit_plan_decode_events_dev
    assert dev_fn(None, 5, 0, count, None, 6, None, None, None, None) == INVALID and "plan" in _err(L)
    assert dev_fn(h, 5, 0, count, None, 6, None, None, None, None) == INVALID and "events" in _err(L)
    assert (p0 == 7).all() and (p1 == 7).all() and (fl == 7).all()      # a refused call wrote nothing
    i8 = lambda a: L.ptr(a, C.c_int8)      # noqa: E731
    s0, s1 = np.zeros((count, 37), np.int8), np.zeros((count, 5), np.int8)
    unpack = lib.qldpc_circuit_plan_unpack_events
    assert unpack(None, count, u8(rec), 6, i8(s0), i8(s1)) == INVALID and "plan" in _err(L)
    assert unpack(h, count, None, 6, i8(s0), i8(s1)) == INVALID and "events" in _err(L)
    assert unpack(h, count, u8(rec), 5, i8(s0), i8(s1)) == INVALID and "stride" in _err(L)
    assert unpack(h, -1, u8(rec), 6, i8(s0), i8(s1)) == INVALID and "count" in _err(L)
    assert unpack(h, count, u8(rec), 6, None, i8(s1)) == INVALID and "sparse0" in _err(L)
    assert unpack(h, count, u8(rec), 6, i8(s0), None) == INVALID and "sparse1" in _err(L)
    layout = lib.qldpc_circuit_plan_set_event_layout
    t0, t1 = L.i32(np.arange(37)), L.i32(37 + np.arange(5))
    i32 = lambda a: L.ptr(a, C.c_int32)      # noqa: E731
    assert layout(None, 42, i32(t0), i32(t1)) == INVALID and "plan" in _err(L)
    for n_bits in (0, -3, 131071):
        assert layout(h, n_bits, i32(t0), i32(t1)) == INVALID and "n_bits" in _err(L)
    assert layout(h, 41, i32(t0), None) == INVALID and "n_bits" in _err(L)          # the default run of sector 1 does not fit
    for tab, row, value in ((0, 36, 42), (0, 0, -2), (1, 4, 42), (1, 2, -2)):
        bad = [t0.copy(), t1.copy()]
        bad[tab][row] = value
        assert layout(h, 42, i32(bad[0]), i32(bad[1])) == INVALID and f"bit_of_row{tab}[{row}]" in _err(L), _err(L)
    # count = 0: QLDPC_OK, nothing touched, whatever the pointers
    assert decode(n=0) == 0 and decode(n=0, events=None, a=None, b=None, f=None) == 0 and (p0 == 7).all() and (fl == 7).all()
    assert unpack(h, 0, None, 6, None, None) == 0
    empty = plan.decode_events(np.zeros((0, 6), np.uint8))
    assert all(x.shape == (0,) for x in empty) and all(x.shape[0] == 0 for x in plan.unpack_events(np.zeros((0, 6), np.uint8)))
    assert not plan.read().any()
    # the refused layouts left the default in place; then a layout set twice: the second one holds, and NULL tables bring the default runs back
    bits = (np.random.default_rng(9).random((count, 64)) < 0.5).astype(np.uint8)
    rec8 = EM.pack(bits)
    n, dflt = EM.default_layout(dem.n_det)
    for got, want in zip(plan.unpack_events(rec8), EM.gather(rec8, n, dflt)):
        assert_same(got, want, "default layout")
    first = [np.arange(37)[::-1].copy(), np.array([40, -1, 40, 63, 0])]
    second = [np.arange(37) + 20, np.array([3, 2, 1, 0, -1])]                       # sector 0: a contiguous run away from its default base
    plan.set_event_layout(64, *first)
    for got, want in zip(plan.unpack_events(rec8), EM.gather(rec8, 64, first)):
        assert_same(got, want, "first layout")
    plan.set_event_layout(64, *second)
    for got, want in zip(plan.unpack_events(rec8), EM.gather(rec8, 64, second)):
        assert_same(got, want, "second layout")
    plan.set_event_layout(64)
    for got, want in zip(plan.unpack_events(rec8), EM.gather(rec8, n, dflt)):
        assert_same(got, want, "default runs of a 64-bit record")
    with pytest.raises(L.QldpcError, match="stride"):           # the layout's n_bits is what stride is held against
        plan.decode_events(np.zeros((count, 6), np.uint8))
    with pytest.raises(ValueError, match="rows0"):
        plan.set_event_layout(64, np.arange(36))
    plan.close()
    # one sector: pred1 may be NULL, and is zeroed when it is not
    z, zg = model(L, DEM, "tiny_z")
    zp = z.plan(zg, max_iter=12, batch=64)
    synd = zp.sample(3, 0, count)[0]
    zrec = EM.pack(synd)
    assert zrec.shape == (count, 5)
    q0, q1, qf = np.zeros(count, np.uint64), np.full(count, 7, np.uint64), np.zeros(count, np.uint8)
    assert lib.qldpc_circuit_plan_decode_events(zp._h, 3, 0, count, u8(zrec), 5, None, u64(q0), None, u8(qf)) == 0, _err(L)
    r0, r1, rf = zp.decode_events(zrec, 3, 0)
    assert np.array_equal(r0, q0) and np.array_equal(rf, qf) and not r1.any() and not (rf & 0x2A).any()
    assert lib.qldpc_circuit_plan_decode_events(zp._h, 3, 0, count, u8(zrec), 5, None, u64(q0), u64(q1), u8(qf)) == 0 and not q1.any()
    assert lib.qldpc_circuit_plan_unpack_events(zp._h, count, u8(zrec), 5, i8(s0), None) == 0 and np.array_equal(s0, synd)
    zp.close()


def test_e5_circuit_plan(L):
    """a plan of qldpc_circuit_plan_create (the bb72 circuit): the records are what sample() calls sparse_z / sparse_x, in that order"""
    from test_relay_gpu import circuit_setup
    c, compiled, M, graphs, priors, masks, make = circuit_setup(L, "circ72")
    plan = make(batch=64, max_iter=12)
    seed, begin, count = 99, 10, 64
    spz, tz, spx, tx = plan.sample(seed, begin, count)
    outcome = plan.run_outcomes(seed, begin, count)
    tally = plan.read(clear=True)
    records = default_records([spz, spx])
    got = plan.unpack_events(records)
    assert assert_same(got[0], spz, "sparse_z") and assert_same(got[1], spx, "sparse_x")
    pred0, pred1, flags = plan.decode_events(records, seed, begin)
    assert_same(verdicts((pred0, pred1), [tz, tx]), outcome, "verdicts")
    assert int((flags & 1).sum()) == tally[L.TALLY["bp_conv_z"]] and int(((flags >> 1) & 1).sum()) == tally[L.TALLY["bp_conv_x"]]
    assert assert_same((flags >> 4) & 1, ~spz.any(axis=1), "zero syndrome Z") and assert_same((flags >> 5) & 1, ~spx.any(axis=1), "zero syndrome X")
    assert not plan.read().any()
    ph, nb = plan.phase_times()                                  # the brackets: sample = copy + unpack, judge = predict, BP as in a run
    assert nb == 2 and ph["sample"] > 0 and ph["judge"] > 0 and ph["bp_z"] > 0 and ph["bp_x"] > 0
    plan.close()


# ---- E6 -----------------------------------------------------------------------------------------------------------------------------------------------
TEXT = """
error(0.1) D0 D1 L0
error(0.05) D1 D2
error(0.1) D2 D3 L1
error(0.02) D3 D4 ^ D5
error(0.1) D5 D6 L2
error(0.03) D6 D7
error(0.1) D7 D8 L0 L2
error(0.04) D8 D9
error(0.1) D9 D10
error(0.06) D10 D11 L1
error(0.05) D0 D11
error(0.07) D4 D6 L0
error(0.07) D3 D7 L2
"""


def test_e6_python_surface(L, DEM, tmp_path):
    from qldpc_amd.simulation.dem import DemDecoder, read_b8
    dem = DEM.from_text(TEXT, sector_of_detector=np.arange(12) % 2)
    assert dem.n_det == (6, 6) and dem.k == (3, 3) and dem.n_detectors == 12
    count, seed = 500, 12
    graphs = [L.Graph(v.indptr, v.indices, v.shape[1]) for v in (dem.decoder_view(0), dem.decoder_view(1))]
    plan = dem.plan(graphs, max_iter=12, batch=128)
    spz, tz, spx, tx = plan.sample(seed, 0, count)
    by_hand = plan.decode_events(default_records([spz, spx]), seed, 0)      # the per-sector syndromes, concatenated by hand
    assert_same(verdicts(by_hand[:2], [tz, tx]), plan.run_outcomes(seed, 0, count), "verdicts")
    plan.close()
    events = np.zeros((count, 12), bool)                        # the same shots in the TEXT's numbering: sector 0 holds D0, D2, ..., sector 1 D1, D3, ...
    events[:, 0::2], events[:, 1::2] = spz != 0, spx != 0
    assert events.any(axis=0).all()
    dec = DemDecoder(dem, maxIter=12, batch=128, seed=seed)
    (a0, a1), flags = dec.decode_to_flags(events)
    assert a0.dtype == np.bool_ and a0.shape == (count, 3) and a1.shape == (count, 3) and flags.shape == (count,)
    assert_same(a0, EM.pred_bits(by_hand[0], 3) != 0, "sector 0 against the plan fed by hand")
    assert_same(a1, EM.pred_bits(by_hand[1], 3) != 0, "sector 1 against the plan fed by hand")
    assert_same(flags, by_hand[2], "flags")
    assert a0.any() and a1.any()
    packed = L.pack_events(events)
    for what, form in (("uint8", events.astype(np.uint8)), ("packed", packed), ("packed, wide stride", np.hstack([packed, np.full((count, 2), 0xFF, np.uint8)]))):
        b0, b1 = dec.decode_batch(form, bit_packed=True if "wide" in what else None)
        assert assert_same(b0, a0, f"{what}: sector 0") and assert_same(b1, a1, f"{what}: sector 1")
    path = tmp_path / "shots.b8"
    packed.tofile(path)
    back = read_b8(path, 12)
    assert np.array_equal(back, packed)
    b0, b1 = dec.decode_batch(back)
    assert assert_same(b0, a0, "read_b8: sector 0") and assert_same(b1, a1, "read_b8: sector 1")
    c0, c1 = dec.decode_batch(events[100:], shot_begin=100)     # a split range (nothing here draws from the index, so the answer is the tail)
    assert assert_same(c0, a0[100:], "tail: sector 0") and assert_same(c1, a1[100:], "tail: sector 1")
    dec.close()
    # one sector: the array itself, column r = L<r>; the switches come with the decoder
    one = DEM.from_text(TEXT)
    d1 = DemDecoder(one, maxIter=12, batch=128, decoder="relay_bp", relay_params=RELAY, seed=seed)
    g1 = [L.Graph(one.decoder_view(0).indptr, one.decoder_view(0).indices, one.decoder_view(0).shape[1])]
    p1 = one.plan(g1, max_iter=12, batch=128)
    p1.use_relay(**RELAY)
    s1, t1 = p1.sample(seed, 0, count)[:2]
    want = p1.decode_events(L.pack_events(s1), seed, 7)
    p1.close()
    out = d1.decode_batch(s1.astype(np.uint8), shot_begin=7)
    d1.close()
    assert isinstance(out, np.ndarray) and out.shape == (count, 3)
    assert_same(out, EM.pred_bits(want[0], 3) != 0, "one sector")
