"""The clean undamped regular min-sum kernel builds its check messages without compares or selects (csrc/minsum_regular.hip: leave-one-out minima from
prefix / suffix chains, the clip in the chain seeds, signs from high words).  Outputs against the C oracle, which clips every edge and selects the first
strict minimum: the decode API on the smallest (6,3) team (bb72) and on one (4,2)- and one (8,4)-regular graph, words of the posteriors included, and
the fused Monte-Carlo plan on inputs that the oracle and the numpy model (tests/clip_minima_model.py) first show to hold BP failures and clipped checks."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import graph_shapes as GS  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_ITER = 50
CLIPS = (20.0, 6.0, 1.0)
DECODE_SHOTS = 256
MC_P, MC_SHOTS, MC_BATCH, MC_SEED, MC_CLIP = 0.02, 20000, 4096, 20261018, 6.0
MC_MODELLED = 1024       # shots of the Monte-Carlo sample that the numpy model decodes to count clipped check updates (the oracle does not count them)


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _syndromes(indptr, indices, errors):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out = np.zeros((errors.shape[0], len(indptr) - 1), np.int64)
    np.add.at(out, (slice(None), rows), errors[:, indices])
    return (out & 1).astype(np.int8)


def _graph(tag):
    """-> (indptr, indices, n, prior error rate, syndrome error rate)"""
    if tag == "bb72":
        from qldpc_amd.data import load_code
        c = load_code("bb72")
        return c["Hx_indptr"], c["Hx_indices"], int(c["n"]), 0.005, 0.03
    cdeg, vdeg, m = {"reg42": (4, 2, 30), "reg84": (8, 4, 45)}[tag]        # team sizes 30 and 45: no multiple of a wave, several shots per workgroup
    n = m * cdeg // vdeg
    ip, ix = GS.deal(np.random.default_rng([20261018, cdeg, 0]), m, np.full(n, vdeg), row_cap=cdeg)
    rd, cd = GS.degrees(ip, ix, n)
    assert GS.regular_takes(rd, cd) and (int(rd.max()), int(cd.max())) == (cdeg, vdeg)
    return ip, ix, n, 0.04, 0.04


@pytest.fixture(scope="module")
def decode_case(L, oracle):
    cache = {}

    def get(tag):
        if tag not in cache:
            ip, ix, n, p, pe = _graph(tag)
            rng = np.random.default_rng(len(tag) + n)
            synd = _syndromes(ip, ix, (rng.random((DECODE_SHOTS, n)) < pe).astype(np.int64))
            cache[tag] = (ip, ix, n, np.full(n, np.log((1 - p) / p)), synd, L.Graph(ip, ix, n))
        return cache[tag]
    return get


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("tag", ["bb72", "reg42", "reg84"])
def test_decode_api_equals_the_oracle(L, oracle, decode_case, tag, clip):
    ip, ix, n, prior, synd, g = decode_case(tag)
    assert L.minsum_decode_path(g, prior, MAX_ITER, "dynamical", 1.0, clip_llr=clip)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=MAX_ITER, clip_llr=clip, threads=0)
    print(f"{tag} clip {clip}: {int(want[1].sum())} of {DECODE_SHOTS} shots converge, iterations up to {int(want[3].max()) + 1}")
    assert 0 < int(want[1].sum()) < DECODE_SHOTS, "the syndromes should hold converging and failing shots"
    for flags, name in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        got = L.minsum_decode_batch(g, synd, prior, MAX_ITER, "dynamical", 1.0, clip_llr=clip, flags=flags)
        for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
            if what == "llr":
                a, b = CM.words(a), CM.words(b)
            bad = np.flatnonzero((np.asarray(a) != np.asarray(b)).reshape(DECODE_SHOTS, -1).any(axis=1))
            assert bad.size == 0, f"{tag} clip {clip} {name}: {what} differs from the oracle on shots {bad[:8].tolist()} ({bad.size} of {DECODE_SHOTS})"


def test_monte_carlo_plan_equals_the_oracle(L, oracle):
    from qldpc_amd.data import load_code
    c = load_code("bb72")
    ip, ix, n = c["Hx_indptr"], c["Hx_indices"], int(c["n"])
    want = oracle.cc_sample_decode_tally(ip, ix, n, c["Lx"], MC_P, MC_SEED, 0, MC_SHOTS, max_iter=MAX_ITER, clip_llr=MC_CLIP, threads=0)
    # the inputs first, on the CPU alone: BP must fail on some shot (the oracle's own tally), and some check update must read an edge the clip
    # changed (the numpy model on the first MC_MODELLED shots, whose verdicts the oracle's tally of those shots confirms)
    failures = int(want[L.TALLY["trials"]] - want[L.TALLY["bp_conv_z"]])
    head = oracle.cc_sample_decode_tally(ip, ix, n, c["Lx"], MC_P, MC_SEED, 0, MC_MODELLED, max_iter=MAX_ITER, clip_llr=MC_CLIP, threads=0)
    errors = np.array([oracle.cc_sample_errors(MC_SEED, b, n, MC_P) for b in range(MC_MODELLED)]).astype(np.int64).reshape(MC_MODELLED, n)
    model = CM.MinSumModel(ip, ix, n).decode(_syndromes(ip, ix, errors), np.full(n, np.log((1 - MC_P) / MC_P)), MAX_ITER, MC_CLIP, "minima")
    assert int(model["conv"].sum()) == int(head[L.TALLY["bp_conv_z"]]) and int(model["iters"].sum()) + MC_MODELLED == int(head[L.TALLY["iters_z"]])
    print(f"bb72 p {MC_P} clip {MC_CLIP}: {failures} BP failures in {MC_SHOTS} shots, {model['clipped_updates']} of {model['updates']} check updates of the "
          f"first {MC_MODELLED} shots had a clipped edge")
    assert failures >= 1 and model["clipped_updates"] >= 1
    g = L.Graph(ip, ix, n)
    for flags, name in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        got = np.zeros_like(want)
        for begin in range(0, MC_SHOTS, MC_BATCH):
            got = got + L.cc_sample_decode_tally(g, c["Lx"], MC_P, MC_SEED, begin, min(MC_BATCH, MC_SHOTS - begin), max_iter=MAX_ITER, clip_llr=MC_CLIP, flags=flags)
        assert np.array_equal(got, want), f"{name}: tally {got.tolist()} != oracle {want.tolist()}"
