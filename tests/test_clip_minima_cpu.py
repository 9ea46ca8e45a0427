"""Clipping the two minima of a check equals clipping each of its edges (clip > 0): message words bit for bit, on random and on constructed
inputs, for the degrees the kernels meet (4, 6, 8: bivariate-bicycle codes; 35: the circuit-level matrices).  The models are
tests/clip_minima_model.py; the kernel that relies on the identity is csrc/minsum_regular.hip (clean undamped path); degree 35 and the first-minimum
selector cover the form the workgroup kernels would take."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402

DEGREES = (4, 6, 8, 35)
CLIPS = (20.0, 6.0, 1.0, 0.37)


def both_forms_agree(t, clip, alpha, synd):
    """edge form == minima form with either selector, as 64-bit words"""
    want = CM.words(CM.check_messages(t, clip, alpha, synd, "edge"))
    for selector in ("equal", "first"):
        got = CM.words(CM.check_messages(t, clip, alpha, synd, "minima", selector))
        bad = np.argwhere(got != want)
        assert bad.size == 0, (selector, clip, alpha, bad[:4].tolist(), np.asarray(t)[tuple(bad[0][:-1])].tolist())


@pytest.mark.parametrize("D", DEGREES)
def test_random_inputs(D):
    rng = np.random.default_rng(1000 + D)
    for clip in CLIPS:
        for scale in (0.3 * clip, clip, 4.0 * clip):                # mostly inside the range, a mix, mostly saturated
            t = rng.normal(0.0, scale, size=(4000, D))
            synd = rng.integers(0, 2, size=4000)
            both_forms_agree(t, clip, float(rng.uniform(0.5, 1.0)), synd)
    # values drawn from a small set: ties everywhere, among them ties at the minimum, at the clip and above it
    for clip in CLIPS:
        pool = np.array([0.0, -0.0, 0.25 * clip, -0.25 * clip, clip, -clip, np.nextafter(clip, np.inf), -np.nextafter(clip, 0.0), 3.0 * clip, -7.0 * clip])
        t = pool[rng.integers(0, len(pool), size=(6000, D))]
        both_forms_agree(t, clip, 0.875, rng.integers(0, 2, size=6000))


@pytest.mark.parametrize("D", DEGREES)
def test_constructed_inputs(D):
    rng = np.random.default_rng(2000 + D)
    for clip in CLIPS:
        above = lambda k: clip * (1.0 + rng.uniform(0.01, 5.0, size=k)) * rng.choice([-1.0, 1.0], size=k)      # noqa: E731
        cases = []
        for pos in range(D):
            for pos2 in range(D):
                if pos2 == pos:
                    continue
                t = above(D); t[pos] = 0.3 * clip; t[pos2] = -0.3 * clip; cases.append(t)                          # a tie at the minimum, opposite signs
                t = above(D); t[pos] = clip; t[pos2] = -clip; cases.append(t)                                      # magnitudes equal to the clip
                t = above(D); t[pos] = 0.0; t[pos2] = -0.0; cases.append(t)                                        # +0.0 and -0.0 tie at the minimum
                t = above(D); t[pos] = -0.0; t[pos2] = 0.5 * clip; cases.append(t)
            t = above(D); cases.append(t)                                                                          # every magnitude above the clip
            t = above(D); t[pos] = 0.4 * clip * rng.choice([-1.0, 1.0]); cases.append(t)                           # exactly one below the clip
            t = above(D); t[pos] = clip; cases.append(t)                                                           # exactly one AT the clip, the rest above
            t = np.full(D, clip); t[pos] = -clip; cases.append(t)                                                  # every magnitude equal to the clip
            t = np.full(D, -0.0); t[pos] = 0.0; cases.append(t)                                                    # zeros only
            t = above(D); t[pos] = np.inf; t[(pos + 1) % D] = -np.inf; cases.append(t)                             # the +-inf of degree-1 checks' columns
        t = np.array(cases)
        for synd in (0, 1):
            both_forms_agree(t, clip, 0.75, np.full(len(t), synd))


def test_degree_one_rows_keep_an_infinite_second_minimum():
    t = np.array([[0.0], [3.0], [-50.0], [np.nan]])
    mask = np.ones((4, 1), bool)
    for synd in (0, 1):
        want = CM.words(CM.check_messages(t, 6.0, 0.75, np.full(4, synd), "edge", mask=mask))
        got = CM.words(CM.check_messages(t, 6.0, 0.75, np.full(4, synd), "minima", "first", mask=mask))
        assert np.array_equal(got, want) and np.all(np.isinf(want.view(np.float64)))


def test_clip_zero_is_outside_the_identity():
    """clip == 0: every clipped value is +-0.0 and counts as non-negative, the unclipped sign does not -- the message words differ (in the sign of a
    zero), which is why the launcher keeps the per-edge form for such a call."""
    t = np.array([[1.0, -2.0, 3.0, 4.0, 5.0, 6.0]])
    edge = CM.words(CM.check_messages(t, 0.0, 0.75, np.array([0]), "edge"))
    mini = CM.words(CM.check_messages(t, 0.0, 0.75, np.array([0]), "minima"))
    assert not np.array_equal(edge, mini)
    assert np.array_equal(edge.view(np.float64), mini.view(np.float64))          # equal as numbers: zeros


@pytest.mark.parametrize("clip", [20.0, 6.0, 1.0])
def test_whole_decodes_agree(clip):
    """the decoder model with either form: same hard decisions, iteration counts and posteriors (words) on a (6,3)-regular graph and on an irregular one"""
    rng = np.random.default_rng(7)
    m, n = 36, 72
    cols = np.array([(np.array([0, 5, 11, 36, 41, 50]) + 7 * i) % n if i % 2 else (np.array([1, 2, 17, 38, 44, 71]) + 5 * i) % n for i in range(m)])
    cols = np.sort(cols, axis=1)
    graphs = [(np.arange(0, 6 * m + 1, 6), cols.reshape(-1), n)]
    ip, ix = [0], []
    for i in range(20):                                                               # irregular: degrees 1 .. 9
        d = 1 + (i * 5) % 9
        ix += sorted(rng.choice(40, size=d, replace=False).tolist()); ip.append(len(ix))
    graphs.append((np.array(ip), np.array(ix), 40))
    for indptr, indices, nn in graphs:
        M = CM.MinSumModel(indptr, indices, nn)
        err = (rng.random((300, nn)) < 0.06).astype(np.int64)
        synd = np.array([[err[b, indices[indptr[i]:indptr[i + 1]]].sum() & 1 for i in range(M.m)] for b in range(300)])
        prior = np.full(nn, np.log(199.0))
        a = M.decode(synd, prior, 30, clip, "edge")
        for selector in ("equal", "first"):
            b = M.decode(synd, prior, 30, clip, "minima", selector)
            for k in ("hard", "iters", "conv"):
                assert np.array_equal(a[k], b[k]), (k, selector)
            assert np.array_equal(CM.words(a["llr"]), CM.words(b["llr"])), selector
        assert a["updates"] > 0
