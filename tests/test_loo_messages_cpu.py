"""The compare-free check update of the clean undamped regular kernel (csrc/minsum_regular.hip): leave-one-out magnitudes from prefix / suffix minima,
the clip in the two chain seeds, signs from high words.  The numpy model tests/loo_messages_model.py implements it word for word; here its message
words equal those of the minima form it replaces (tests/clip_minima_model.py, form "minima") and of the reference's per-edge form, bit for bit, and
whole decodes through it equal the C oracle.  Inputs follow the kernel's precondition: no value is -0.0 or NaN and clip > 0 (the last test shows that
a -0.0 is indeed outside the identity)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import loo_messages_model as LM  # noqa: E402

DEGREES = (4, 6, 8)
CLIPS = (20.0, 6.0, 1.0)


def agrees(t, clip, alpha, synd):
    """loo form == minima form (the |t| == min1 selector) == per-edge form, as 64-bit words; clip None: iteration 0, no clip"""
    t = np.asarray(t, np.float64)
    assert not (np.signbit(t) & (t == 0)).any() and not np.isnan(t).any()
    got = CM.words(LM.loo_messages(t, clip, alpha, synd))
    if clip is None:
        wants = {"unclipped": CM._messages(t, np.ones(t.shape, bool), synd, alpha, None, "first")}
    else:
        wants = {"minima": CM.check_messages(t, clip, alpha, synd, "minima"), "edge": CM.check_messages(t, clip, alpha, synd, "edge")}
    for name, want in wants.items():
        bad = np.argwhere(got != CM.words(want))
        assert bad.size == 0, (name, clip, alpha, bad[:4].tolist(), t[tuple(bad[0][:-1])].tolist())


@pytest.mark.parametrize("D", DEGREES)
def test_random_inputs(D):
    rng = np.random.default_rng(3000 + D)
    for clip in CLIPS:
        for scale in (0.3 * clip, clip, 4.0 * clip):                # mostly inside the range, a mix, mostly saturated
            t = rng.normal(0.0, scale, size=(4000, D))
            agrees(t, clip, float(rng.uniform(0.5, 1.0)), rng.integers(0, 2, size=4000))
        # values drawn from a small set: ties everywhere, among them ties at the minimum, at the clip and above it, and zeros
        pool = np.array([0.0, 0.25 * clip, -0.25 * clip, clip, -clip, np.nextafter(clip, np.inf), -np.nextafter(clip, 0.0), 3.0 * clip, -7.0 * clip])
        t = pool[rng.integers(0, len(pool), size=(6000, D))]
        agrees(t, clip, 0.875, rng.integers(0, 2, size=6000))
    t = rng.normal(0.0, 5.0, size=(4000, D))                          # iteration 0: no clip
    agrees(t, None, 0.5, rng.integers(0, 2, size=4000))
    t = np.array([0.0, 1.5, -1.5, 40.0, -40.0])[rng.integers(0, 5, size=(4000, D))]
    agrees(t, None, 0.5, rng.integers(0, 2, size=4000))


@pytest.mark.parametrize("D", DEGREES)
def test_constructed_inputs(D):
    rng = np.random.default_rng(4000 + D)
    for clip in CLIPS:
        above = lambda k: clip * (1.0 + rng.uniform(0.01, 5.0, size=k)) * rng.choice([-1.0, 1.0], size=k)      # noqa: E731
        cases = []
        for pos in range(D):
            for pos2 in range(D):
                if pos2 == pos:
                    continue
                t = above(D); t[pos] = 0.3 * clip; t[pos2] = -0.3 * clip; cases.append(t)                          # the minimum attained twice, opposite signs
                pos3 = next(p for p in range(D) if p not in (pos, pos2))
                t = above(D); t[pos] = 0.3 * clip; t[pos2] = -0.3 * clip; t[pos3] = 0.3 * clip; cases.append(t)    # ... and three times
                t = above(D); t[pos] = clip; t[pos2] = -clip; cases.append(t)                                      # magnitudes equal to the clip
                t = above(D); t[pos] = 0.0; t[pos2] = 0.5 * clip; cases.append(t)                                  # a zero magnitude, unique minimum
                t = above(D); t[pos] = 0.0; t[pos2] = 0.0; cases.append(t)                                         # two zeros
                t = above(D); t[pos] = 0.2 * clip; t[pos2] = -0.6 * clip; cases.append(t)                          # min1 and min2 both below the clip
            t = above(D); cases.append(t)                                                                          # every magnitude above the clip
            t = above(D); t[pos] = 0.4 * clip * rng.choice([-1.0, 1.0]); cases.append(t)                           # exactly one below the clip
            t = above(D); t[pos] = clip; cases.append(t)                                                           # exactly one AT the clip, the rest above
            t = np.full(D, 0.7 * clip); t[pos] = -0.7 * clip; cases.append(t)                                      # all magnitudes equal, below the clip
            t = np.full(D, clip); t[pos] = -clip; cases.append(t)                                                  # ... equal to the clip
            t = np.full(D, 3.0 * clip); t[pos] = -3.0 * clip; cases.append(t)                                      # ... above the clip
            t = np.zeros(D); cases.append(t)                                                                       # zeros only
        t = np.array(cases)
        for synd in (0, 1):
            agrees(t, clip, 0.75, np.full(len(t), synd))
            agrees(t, None, 0.75, np.full(len(t), synd))                                                           # the same rows at iteration 0: no clip


def test_the_model_has_no_selector():
    """min over the other edges, written out: position k gets min2 exactly where the minimum is attained once, min1 everywhere else"""
    t = np.array([[3.0, -1.0, 2.0, 5.0], [1.0, -1.0, 2.0, 5.0], [4.0, 4.0, -4.0, 4.0]])
    mags = np.abs(LM.loo_messages(t, 20.0, 1.0, np.zeros(3, int)))
    assert mags.tolist() == [[1.0, 2.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [4.0, 4.0, 4.0, 4.0]]
    signs = np.signbit(LM.loo_messages(t, 20.0, 1.0, np.array([0, 1, 0])))
    assert signs.tolist() == [[True, False, True, True], [False, True, False, False], [True, True, False, True]]


def test_minus_zero_is_outside_the_identity():
    """a -0.0 input counts as >= 0 in the reference and as negative in the high-word form: the kernel's clean inputs exclude it (no posterior and no
    V - R is -0.0), the NaN-tolerant kernel keeps the compares"""
    t = np.array([[-0.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    want = CM.words(CM.check_messages(t, 20.0, 0.75, np.array([0]), "edge"))
    got = CM.words(LM.loo_messages(t, 20.0, 0.75, np.array([0])))
    assert not np.array_equal(got, want)


def _syndromes(indptr, indices, errors):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out = np.zeros((errors.shape[0], len(indptr) - 1), np.int64)
    np.add.at(out, (slice(None), rows), errors[:, indices])
    return (out & 1).astype(np.int8)


@pytest.fixture(scope="module")
def decode_inputs():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    out = {}
    for tag in ("bb72", "bb144"):
        c = load_code(tag)
        ip, ix, n = c["Hx_indptr"], c["Hx_indices"], int(c["n"])
        rng = np.random.default_rng(72 if tag == "bb72" else 144)
        synd = _syndromes(ip, ix, (rng.random((192, n)) < 0.05).astype(np.int64))
        out[tag] = (ip, ix, n, synd, LM.LooModel(ip, ix, n))
    return out


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("tag", ["bb72", "bb144"])
def test_whole_decodes_equal_the_oracle(oracle, decode_inputs, tag, clip):
    ip, ix, n, synd, model = decode_inputs[tag]
    prior = np.full(n, np.log((1 - 0.005) / 0.005))
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=50, clip_llr=clip, threads=0)
    got = model.decode(synd, prior, 50, clip)
    assert 0 < int(want[1].sum()) < len(synd), "the syndromes should hold converging and failing shots"
    assert np.array_equal(got["hard"], want[0])
    assert np.array_equal(got["conv"], want[1])
    assert np.array_equal(got["iters"], want[3])
    assert np.array_equal(CM.words(got["llr"]), CM.words(want[2]))
