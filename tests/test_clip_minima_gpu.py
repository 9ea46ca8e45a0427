"""The clean regular min-sum kernel clips a check's two minima instead of its edges (csrc/minsum_regular.hip): bit-equality with the C
oracle, which clips every edge, at clips that saturate -- the numpy model (tests/clip_minima_model.py) counts, on the same syndromes, how many check
updates had an edge the clip changed, so that a pass cannot come from inputs that never clip."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu

P = 0.005                                   # prior log(199) ~ 5.29: clip 1.0 saturates every edge from iteration 1 on, clip 6.0 gives a mix
MAX_ITER = 50
CLIPS = (20.0, 6.0, 1.0)
MIN_CLIPPED_SHARE = 0.5                     # of the check updates that read clipped values, for the clips 6.0 and 1.0
DECODE_SHOTS, DECODE_ERROR_RATE = 768, 0.02
MC_SHOTS, MC_SEED = 6144, 20261017


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _code(L, tag):
    from qldpc_amd.data import load_code
    c = load_code(tag)
    ip, ix, n = c["Hx_indptr"], c["Hx_indices"], int(c["n"])
    return c, ip, ix, n, L.Graph(ip, ix, n)


def _syndromes(indptr, indices, errors):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out = np.zeros((errors.shape[0], len(indptr) - 1), np.int64)
    np.add.at(out, (slice(None), rows), errors[:, indices])
    return (out & 1).astype(np.int8)


def _assert_decode_equal(got, want, what):
    for name, a, b in zip(("hard decisions", "converged", "llr", "iterations"), got, want):
        if name == "llr":
            a, b = CM.words(a), CM.words(b)
        bad = np.flatnonzero((np.asarray(a) != np.asarray(b)).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differ from the oracle on shots {bad[:8].tolist()} ({bad.size} of {len(a)})"


def _share(model_out, what, clip):
    share = model_out["clipped_updates"] / max(model_out["updates"], 1)
    print(f"{what} clip {clip}: {model_out['clipped_updates']} of {model_out['updates']} check updates had a clipped edge ({share:.3f})")
    return share


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("tag", ["bb72", "bb144", "bb288"])
def test_decode_mode_equals_the_oracle(L, oracle, tag, clip):
    c, ip, ix, n, g = _code(L, tag)
    rng = np.random.default_rng(144)
    synd = _syndromes(ip, ix, (rng.random((DECODE_SHOTS, n)) < DECODE_ERROR_RATE).astype(np.int64))
    prior = np.full(n, np.log((1 - P) / P))
    assert L.minsum_decode_path(g, prior, MAX_ITER, "dynamical", 1.0, clip_llr=clip)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=MAX_ITER, clip_llr=clip, threads=0)
    model = CM.MinSumModel(ip, ix, n).decode(synd, prior, MAX_ITER, clip, "minima")
    assert np.array_equal(model["hard"], want[0]) and np.array_equal(model["iters"], want[3]) and np.array_equal(CM.words(model["llr"]), CM.words(want[2]))
    share = _share(model, f"{tag} decode", clip)
    if clip < 20.0:
        assert share >= MIN_CLIPPED_SHARE
    for flags, name in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        got = L.minsum_decode_batch(g, synd, prior, MAX_ITER, "dynamical", 1.0, clip_llr=clip, flags=flags)
        _assert_decode_equal(got, want, f"{tag} clip {clip} {name}")


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("tag", ["bb72", "bb144", "bb288"])
def test_fused_monte_carlo_equals_the_oracle(L, oracle, tag, clip):
    c, ip, ix, n, g = _code(L, tag)
    want = oracle.cc_sample_decode_tally(ip, ix, n, c["Lx"], P, MC_SEED, 0, MC_SHOTS, max_iter=MAX_ITER, clip_llr=clip, threads=0)
    errors = np.array([oracle.cc_sample_errors(MC_SEED, b, n, P) for b in range(MC_SHOTS)]).astype(np.int64).reshape(MC_SHOTS, n)
    synd = _syndromes(ip, ix, errors)
    prior = np.full(n, np.log((1 - P) / P))
    model = CM.MinSumModel(ip, ix, n).decode(synd, prior, MAX_ITER, clip, "minima")
    assert int(model["conv"].sum()) == int(want[L.TALLY["bp_conv_z"]]) and int(model["iters"].sum()) + MC_SHOTS == int(want[L.TALLY["iters_z"]])
    share = _share(model, f"{tag} Monte-Carlo", clip)
    if clip < 20.0:
        assert share >= MIN_CLIPPED_SHARE
    for flags, name in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        got = L.cc_sample_decode_tally(g, c["Lx"], P, MC_SEED, 0, MC_SHOTS, max_iter=MAX_ITER, clip_llr=clip, flags=flags)
        assert np.array_equal(got, want), f"{tag} clip {clip} {name}: tally {got.tolist()} != oracle {want.tolist()}"


@pytest.mark.parametrize("tag", ["bb72", "bb144", "bb288"])
def test_clip_zero_takes_the_per_edge_form(L, oracle, tag):
    """clip_llr = 0 is outside the identity (tests/test_clip_minima_cpu.py::test_clip_zero_is_outside_the_identity): such a call is not "clean", the
    launcher gives it the NaN-tolerant kernel, which clips every edge, and the outputs equal the oracle's in both modes."""
    c, ip, ix, n, g = _code(L, tag)
    rng = np.random.default_rng(5)
    synd = _syndromes(ip, ix, (rng.random((256, n)) < DECODE_ERROR_RATE).astype(np.int64))
    prior = np.full(n, np.log((1 - P) / P))
    assert L.minsum_decode_path(g, prior, MAX_ITER, "dynamical", 1.0, clip_llr=0.0)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=MAX_ITER, clip_llr=0.0, threads=0)
    for flags, name in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        got = L.minsum_decode_batch(g, synd, prior, MAX_ITER, "dynamical", 1.0, clip_llr=0.0, flags=flags)
        _assert_decode_equal(got, want, f"{tag} clip 0 {name}")
        t_got = L.cc_sample_decode_tally(g, c["Lx"], P, MC_SEED, 0, 2048, max_iter=MAX_ITER, clip_llr=0.0, flags=flags)
        t_want = oracle.cc_sample_decode_tally(ip, ix, n, c["Lx"], P, MC_SEED, 0, 2048, max_iter=MAX_ITER, clip_llr=0.0, threads=0)
        assert np.array_equal(t_got, t_want), f"{tag} clip 0 {name}: tally {t_got.tolist()} != oracle {t_want.tolist()}"
