"""Min-sum with a per-shot prior (csrc/shot_prior.hip) on the GPU: word for word the decimation kernel with nothing to freeze and bit for bit the numpy
model (tests/correlated_model.py) on the families of tests/leg_shapes.py; per-shot priors against the model and against one call per shot; the link
tables through prior_out; the three storage modes on families sized by the restated rule, with the accept / refuse line observed by the return code;
every refusal of the C ABI; and the device entry against the host entry.

What is observed and what is not: the ABI does not report where V and P live, so on the two lines between the storage modes this module asserts
bit-equality with the model on both sides and nothing else; the line between "both in global memory" and "refused" is observed directly."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402
import graph_shapes as GS  # noqa: E402
import leg_shapes as LS  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("err", "llr", "conv", "iters")
CASES = LS.all_cases()
BY_NAME = {c.name: c for c in CASES}
DECIM_CASES = [c.name for c in CASES if LS.modes(c)[0]]
SETS = (dict(alpha=0.875, clip_llr=20.0, max_iter=9), dict(alpha=1.0, clip_llr=6.5, max_iter=30))
_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def graph_of(L, name, ip, ix, n):
    """one handle per graph for the whole module"""
    if name not in _GRAPHS:
        _GRAPHS[name] = L.Graph(ip, ix, n)
    return _GRAPHS[name]


def assert_same(got, ref, what):
    for a, b, name in zip(got, ref, NAMES + ("prior_out",)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} has another type or shape"
        if name == "llr":
            assert np.array_equal(a, b, equal_nan=True), f"{what}: llr differs"         # bytes, NaN payloads aside
            assert np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])), f"{what}: a zero of llr has another sign"
        else:
            assert a.tobytes() == b.tobytes(), f"{what}: {name} differs"


def rng_of(name):
    return np.random.default_rng([20261020, zlib.crc32(name.encode())])


def random_links(rng, n, n_src, per_col=2, heavy=None):
    """about per_col links on a third of the columns, llr of either sign; heavy {column: links} on top.  -> (ptr, src, llr)"""
    counts = np.where(rng.random(n) < 1 / 3, rng.integers(1, per_col + 1, n), 0)
    for j, k in (heavy or {}).items():
        counts[j] = k
    counts = np.minimum(counts, n_src)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    src = np.concatenate([np.sort(rng.choice(n_src, k, replace=False)) for k in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, src, np.round(rng.normal(0.5, 3.0, src.size), 3)


# ---------------------------------------------------------------------------------------- 1. against an existing kernel
def test_the_case_list_is_the_one_bpgd_accepts():
    assert set(DECIM_CASES) == set(BY_NAME) - {"decim_refused", "relay_vg_last", "relay_refused"}
    for name in DECIM_CASES:
        c = BY_NAME[name]
        assert CM.shotprior_mode(c.m, c.n, int(c.row_deg.max())) != 0


@pytest.mark.parametrize("name", DECIM_CASES)
def test_shared_prior_equals_decimation_without_rounds_and_the_model(L, name):
    c = BY_NAME[name]
    g, synd = graph_of(L, name, c.indptr, c.indices, c.n), LS.syndromes(c)
    for pn, prior in c.priors.items():
        for p in SETS[:1] if c.n > 3000 else SETS:
            got = L.shotprior_decode_batch(g, synd, prior, **p)
            dec = L.decim_decode_batch(g, synd, prior, alpha=p["alpha"], clip_llr=p["clip_llr"], t_round=p["max_iter"], max_rounds=0, per_round=1, fix_llr=50.0)
            assert_same(got, dec[:4], f"{name} / {pn}: against qldpc_decim_decode_batch")
            assert_same(got, CM.decode(c.indptr, c.indices, c.n, synd, prior, **p), f"{name} / {pn}: against the model")


# ---------------------------------------------------------------------------------------- 2. per-shot priors
@pytest.mark.parametrize("name", ["n33", "small_irregular", "block_513_4096"])
def test_per_shot_priors(L, name):
    c = BY_NAME[name]
    g = graph_of(L, name, c.indptr, c.indices, c.n)
    rng = rng_of("per shot/" + name)
    synd = np.concatenate([LS.syndromes(c), GS.syndromes(c, 4, salt=1)])
    B = synd.shape[0]
    assert B == 8
    priors = rng.normal(2.5, 2.0, (B, c.n))
    priors[:, ::7] = rng.choice([-31.5, 27.0, 44.25], (B, len(range(0, c.n, 7))))      # magnitudes above clip_llr = 20, of either sign
    assert (priors < 0).any() and (np.abs(priors) > 20.0).any()
    p = SETS[0]
    got = L.shotprior_decode_batch(g, synd, priors, want_prior=True, **p)
    assert_same(got[:4], CM.decode(c.indptr, c.indices, c.n, synd, priors, **p), f"{name}: against the model")
    assert got[4].tobytes() == priors.tobytes()
    for b in range(B):
        one = L.shotprior_decode_batch(g, synd[b:b + 1], priors[b], **p)
        assert_same([a[b:b + 1] for a in got[:4]], one, f"{name}: shot {b} against its own stride-0 call")


# ---------------------------------------------------------------------------------------- 3. links
def test_reweight_edge_cases_through_prior_out(L):
    ip, ix = GS.deal(rng_of("edge/graph"), 3, np.full(4, 2))
    g = graph_of(L, "edge", ip, ix, 4)
    ptr, src, llr = [0, 2, 2, 3, 4], [0, 4, 2, 1], [1.5, -0.25, 9.0, -7.0]
    base = np.array([3.0, 2.0, 4.0, 0.5])
    fired = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 1], [1, 0, 1, 0, 0], [0, 1, 0, 0, 1], [2, 2, 2, 2, 2]], np.int8)
    synd = np.zeros((5, 3), np.int8)
    got = L.shotprior_decode_batch(g, synd, base, links=(ptr, src, llr), src_err=fired, want_prior=True, **SETS[0])
    assert got[4].tolist() == [[3.0, 2.0, 4.0, 0.5], [-0.25, 2.0, 4.0, 0.5], [1.5, 2.0, 4.0, 0.5], [-0.25, 2.0, 4.0, -7.0], [3.0, 2.0, 4.0, 0.5]]
    assert got[4].tobytes() == CM.reweight(base, fired, ptr, src, llr).tobytes()
    assert_same(got[:4], CM.decode(ip, ix, 4, synd, got[4], **SETS[0]), "edge cases")
    # no tables, and tables with nothing in them: the prior as given
    for kw in (dict(), dict(links=([0, 0, 0, 0, 0], [], []), src_err=fired)):
        assert L.shotprior_decode_batch(g, synd, base, want_prior=True, **kw, **SETS[0])[4].tobytes() == np.tile(base, (5, 1)).tobytes()


@pytest.mark.parametrize("name", ["n1", "n31", "n32", "n33", "few_hundred"])
def test_links_equal_the_model(L, name):
    rng = rng_of("links/" + name)
    if name == "few_hundred":
        n, n_src = 300, 211
        ip, ix = GS.deal(rng_of("few_hundred/graph"), 60, np.full(n, 3))
        c = LS._case(name, ip, ix, n, {}, {}, err_weight=4)
        heavy = {17: 150, 299: 65}                                         # more links than a wave has lanes
    else:
        c = BY_NAME[name]
        n, n_src, heavy = c.n, 70, {0: 66}
    g = graph_of(L, name, c.indptr, c.indices, c.n)
    ptr, src, llr = random_links(rng, n, n_src, heavy=heavy)
    assert np.diff(ptr).max() > 64
    B = 8
    synd = np.concatenate([GS.syndromes(c, 4), GS.syndromes(c, 4, salt=1)])
    fired = (rng.random((B, n_src)) < 0.15).astype(np.int8)
    fired[0] = 0
    fired[1] = 1
    for prior in (rng.normal(2.5, 1.5, n), rng.normal(2.5, 1.5, (B, n))):
        P = CM.reweight(prior, fired, ptr, src, llr)
        assert (P != np.broadcast_to(prior, (B, n))).any()
        for p in SETS:
            got = L.shotprior_decode_batch(g, synd, prior, links=(ptr, src, llr), src_err=fired, want_prior=True, **p)
            assert got[4].tobytes() == P.tobytes(), f"{name}: prior_out"
            assert_same(got[:4], CM.decode(c.indptr, c.indices, n, synd, P, **p), f"{name}: against the model")


def test_the_queue_hands_out_a_second_shot(L):
    """B = 1504 is above the largest grid of a 512-thread kernel (256 compute units x at most 4 workgroups): some workgroup takes a second shot from the
    atomic queue and must refill V and P and reset its flags.  The shots are eight in 188 different orders, so every row has a B = 8 row to equal."""
    n, n_src = 300, 211
    ip, ix = GS.deal(rng_of("few_hundred/graph"), 60, np.full(n, 3))
    g = graph_of(L, "few_hundred", ip, ix, n)
    c = LS._case("few_hundred", ip, ix, n, {}, {}, err_weight=4)
    assert LS.block_threads(c.m, c.n) == 512
    rng = rng_of("queue")
    synd = np.concatenate([GS.syndromes(c, 4), GS.syndromes(c, 4, salt=1)])
    ptr, src, llr = random_links(rng, n, n_src)
    fired = (rng.random((8, n_src)) < 0.15).astype(np.int8)
    priors = rng.normal(2.5, 1.5, (8, n))
    order = np.concatenate([rng.permutation(8) for _ in range(188)])
    small = L.shotprior_decode_batch(g, synd, priors, links=(ptr, src, llr), src_err=fired, want_prior=True, **SETS[0])
    assert_same(small[:4], CM.decode(ip, ix, n, synd, small[4], **SETS[0]), "B = 8 against the model")
    big = L.shotprior_decode_batch(g, synd[order], priors[order], links=(ptr, src, llr), src_err=fired[order], want_prior=True, **SETS[0])
    assert_same(big, [a[order] for a in small], "B = 1504 against B = 8")


# ---------------------------------------------------------------------------------------- 4. the three storage modes
def _last(ok, lo, hi):
    x = max(v for v in range(lo, hi) if ok(v))
    assert x + 1 < hi and not ok(x + 1)
    return x


def storage_families():
    """(name, indptr, indices, n, mode): the last size of a mode and the first of the next, on each of the three lines of the restated rule.  Columns: m = 300,
    3000 columns with edges and the rest of degree 0, as the *_lds_* families of tests/leg_shapes.py.  Rows: n = 64, 200 rows of degree 5, the rest empty."""
    out = []
    m = 300
    for line, p_lds in (("p", True), ("v", False)):
        n_last = _last(lambda n: CM.shotprior_lds_bytes(m, n, False, p_lds) <= CM.LDS_BYTES, 5000, 30000)
        cd = np.append(GS.blocks(rng_of(line + "/cd"), (4, 1500), (2, 1500), (0, n_last - 3000)), 0)
        for n in (n_last, n_last + 1):
            ip, ix = GS.deal(rng_of(line + "/graph"), m, cd[:n])
            out.append((f"{line}_lds_{n}", ip, ix, n, CM.shotprior_mode(m, n, int(np.diff(ip).max()))))
    n = 64
    m_last = _last(lambda m: CM.shotprior_lds_bytes(m, n, True, False) <= CM.LDS_BYTES, 4000, 9000)
    full = np.sort(rng_of("rows").choice(m_last, 200, replace=False))
    for m in (m_last, m_last + 1):
        empty = {i: [] for i in np.setdiff1d(np.arange(m), full).tolist()}
        cd = np.full(n, 15)
        cd[rng_of("rows/cd").choice(n, 40, replace=False)] = 16
        ip, ix = GS.deal(rng_of("rows/graph"), m, cd, fixed=empty, row_cap=5)
        out.append((f"rows_{m}", ip, ix, n, CM.shotprior_mode(m, n, 5)))
    return out


STORAGE = storage_families()


def test_the_storage_families_sit_on_the_three_lines():
    assert [f[4] for f in STORAGE] == [1, 2, 2, 3, 3, 0]


@pytest.mark.parametrize("fam", STORAGE, ids=[f[0] for f in STORAGE])
def test_storage_modes(L, fam):
    name, ip, ix, n, mode = fam
    g = graph_of(L, name, ip, ix, n)
    c = LS._case(name, ip, ix, n, {}, {}, err_weight=6)
    rng = rng_of("storage/" + name)
    synd = GS.syndromes(c, 4)
    n_src = 50
    ptr, src, llr = random_links(rng, n, n_src)
    fired = (rng.random((4, n_src)) < 0.3).astype(np.int8)
    prior = rng.normal(3.0, 1.0, n)
    p = SETS[0]
    if mode == 0:
        e, c_, i_ = np.full((4, n), 9, np.int8), np.full(4, 9, np.uint8), np.full(4, -7, np.int32)
        for tabs in ((0, None, None, None, None), (n_src, L.ptr(fired, C.c_int8), L.ptr(ptr, C.c_int32), L.ptr(src, C.c_int32), L.ptr(llr, C.c_double))):
            rc = L.lib().qldpc_shotprior_decode_batch(g.handle, 4, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), 0, *tabs, p["alpha"], p["clip_llr"],
                                                      p["max_iter"], L.ptr(e, C.c_int8), None, L.ptr(c_, C.c_uint8), L.ptr(i_, C.c_int32), None)
            assert rc == -4 and b"row degree" in L.lib().qldpc_last_error()
        assert (e == 9).all() and (c_ == 9).all() and (i_ == -7).all()
        return
    P = CM.reweight(prior, fired, ptr, src, llr)
    got = L.shotprior_decode_batch(g, synd, prior, links=(ptr, src, llr), src_err=fired, want_prior=True, **p)
    assert got[4].tobytes() == P.tobytes()
    assert_same(got[:4], CM.decode(ip, ix, n, synd, P, **p), f"{name}: with links")
    assert_same(L.shotprior_decode_batch(g, synd, prior, **p), CM.decode(ip, ix, n, synd, prior, **p), f"{name}: without links")


def test_refused_graphs(L):
    """row degree 57 and a graph without slot tables (n = 65535); row degree 56 is taken"""
    synd = np.zeros((1, 2), np.int8)
    for name, n, deg, ok in (("deg56", 60, 56, True), ("deg57", 60, 57, False), ("wide", 65535, 3, False)):
        ip, ix = np.array([0, deg, deg + 2], np.int32), np.concatenate([np.arange(deg), [0, n - 1]]).astype(np.int32)
        g = graph_of(L, name, ip, ix, n)
        assert (CM.shotprior_mode(2, n, deg) != 0) == ok
        if ok:
            assert_same(L.shotprior_decode_batch(g, synd, np.full(n, 2.0), **SETS[0]), CM.decode(ip, ix, n, synd, np.full(n, 2.0), **SETS[0]), name)
        else:
            with pytest.raises(L.QldpcError, match=r"error -4: .*row degree"):
                L.shotprior_decode_batch(g, synd, np.full(n, 2.0), **SETS[0])


# ---------------------------------------------------------------------------------------- 5. validation
def test_every_refusal_of_the_host_entry(L):
    c = BY_NAME["n33"]
    g = graph_of(L, "n33", c.indptr, c.indices, c.n)
    n, m, B, n_src = c.n, c.m, 2, 5
    synd = np.zeros((B, m), np.int8)
    good = dict(prior=np.full((B, n), 2.0), stride=n, n_src=n_src, src_err=np.zeros((B, n_src), np.int8),
                ptr=np.concatenate([[0, 2], np.full(n - 1, 3)]).astype(np.int32), src=np.array([1, 4, 0], np.int32), llr=np.array([1.0, -2.0, 0.5]),
                alpha=1.0, clip=20.0, max_iter=5)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        out = dict(err=np.full((B, n), 9, np.int8), llr=np.full((B, n), 9.0), conv=np.full(B, 9, np.uint8), iters=np.full(B, -7, np.int32),
                   pout=np.full((B, n), 9.0))
        opt = lambda x, t: L.ptr(np.ascontiguousarray(x), t) if x is not None else None
        keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None for k in ("prior", "src_err", "ptr", "src", "llr")]
        rc = L.lib().qldpc_shotprior_decode_batch(g.handle, B, L.ptr(synd, C.c_int8), opt(keep[0], C.c_double), a["stride"], a["n_src"], opt(keep[1], C.c_int8),
                                                  opt(keep[2], C.c_int32), opt(keep[3], C.c_int32), opt(keep[4], C.c_double), a["alpha"], a["clip"], a["max_iter"],
                                                  L.ptr(out["err"], C.c_int8), L.ptr(out["llr"], C.c_double), L.ptr(out["conv"], C.c_uint8),
                                                  L.ptr(out["iters"], C.c_int32), L.ptr(out["pout"], C.c_double))
        untouched = (out["err"] == 9).all() and (out["llr"] == 9.0).all() and (out["conv"] == 9).all() and (out["iters"] == -7).all() and (out["pout"] == 9.0).all()
        return rc, L.lib().qldpc_last_error().decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    bad_prior = good["prior"].copy()
    bad_prior[1, 7] = np.inf
    ptr_down = good["ptr"].copy()
    ptr_down[5] = 2
    refusals = [
        (dict(stride=1), "prior_stride = 1"), (dict(stride=2 * n), "prior_stride"), (dict(prior=bad_prior), f"prior[{n + 7}]"),
        (dict(llr=np.array([1.0, np.nan, 0.5])), "link_llr[1]"), (dict(ptr=good["ptr"] + 1), "link_ptr[0] = 1"), (dict(ptr=ptr_down), "link_ptr[5] = 2"),
        (dict(src=np.array([1, 5, 0], np.int32)), "link_src[1] = 5"), (dict(src=np.array([-1, 4, 0], np.int32)), "link_src[0] = -1"),
        (dict(src=np.array([4, 1, 0], np.int32)), "link_src[1] = 1"), (dict(src=np.array([1, 1, 0], np.int32)), "link_src[1] = 1"),
        (dict(src_err=None), "all NULL or all given"), (dict(llr=None), "all NULL or all given"), (dict(ptr=None, src=None), "all NULL or all given"),
        (dict(n_src=-1), "n_src = -1"), (dict(alpha=0.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(clip=float("inf")), "clip_llr"),
        (dict(clip=-1.0), "clip_llr"), (dict(max_iter=0), "max_iter"),
    ]
    for kw, text in refusals:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and text in msg and untouched, (kw, msg)


# ---------------------------------------------------------------------------------------- 6. the device entry
def test_device_entry_and_batch_splits(L):
    n, n_src, B = 300, 211, 96
    ip, ix = GS.deal(rng_of("few_hundred/graph"), 60, np.full(n, 3))
    g = graph_of(L, "few_hundred", ip, ix, n)
    c = LS._case("few_hundred", ip, ix, n, {}, {}, err_weight=4)
    rng = rng_of("dev")
    synd = np.concatenate([GS.syndromes(c, 4, salt=s) for s in range(B // 4)])
    ptr, src, llr = random_links(rng, n, n_src, heavy={3: 70})
    fired = (rng.random((B, n_src)) < 0.1).astype(np.int8)
    priors = rng.normal(2.5, 1.5, (B, n))
    p = SETS[0]
    host = L.shotprior_decode_batch(g, synd, priors, links=(ptr, src, llr), src_err=fired, want_prior=True, **p)
    assert_same(host[:4], CM.decode(ip, ix, n, synd, host[4], **p), "host entry against the model")
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(synd=up(synd), prior=up(priors), fired=up(fired), ptr=up(ptr), src=up(src), llr=up(llr))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(lo, hi, with_llr=True):
        k = hi - lo
        out = (torch.zeros((k, n), dtype=torch.int8, device=dev), torch.full((k, n), -7.0, dtype=torch.float64, device=dev),
               torch.zeros(k, dtype=torch.uint8, device=dev), torch.zeros(k, dtype=torch.int32, device=dev), torch.full((k, n), -7.0, dtype=torch.float64, device=dev))
        L.check(L.lib().qldpc_shotprior_decode_batch_dev(g.handle, k, d["synd"][lo:hi].data_ptr(), d["prior"][lo:hi].data_ptr(), n, n_src, d["fired"][lo:hi].data_ptr(),
                                                         d["ptr"].data_ptr(), d["src"].data_ptr(), d["llr"].data_ptr(), p["alpha"], p["clip_llr"], p["max_iter"],
                                                         out[0].data_ptr(), out[1].data_ptr() if with_llr else None, out[2].data_ptr(), out[3].data_ptr(),
                                                         out[4].data_ptr() if with_llr else None, stream))
        torch.cuda.synchronize(dev)
        return [t.cpu().numpy() for t in out]

    whole = run(0, B)
    assert_same(whole, host, "one device call of 96 against the host entry")
    parts = [run(lo, lo + 32) for lo in (0, 32, 64)]
    assert_same([np.concatenate([q[i] for q in parts]) for i in range(5)], whole, "three device calls of 32 against one of 96")
    bare = run(0, 32, with_llr=False)                                      # llr = prior_out = NULL: nothing is written in their place
    assert_same([bare[0], parts[0][1], bare[2], bare[3]], parts[0][:4], "device entry with NULL llr and prior_out")
    assert (bare[1] == -7.0).all() and (bare[4] == -7.0).all()
