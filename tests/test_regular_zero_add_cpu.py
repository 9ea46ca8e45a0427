"""The claim behind the variable sum of the clean regular min-sum forms (csrc/minsum_regular.hip), without a GPU.

"zero" (header comment): the reference's variable sum is (((0.0 + a) + b) + c) + prior; the clean forms compute ((a + b) + c) + prior.  For a prior that is
not -0.0 the posterior WORD is the same: the running sums differ only while every addend so far is -0.0 (+0.0 against -0.0), and adding the prior
closes that gap.  Checked bit for bit over every ordered triple of messages drawn from +-0.0, random doubles (both signs, wide exponent range, pairs
that cancel exactly) and multiples of 1/8, against priors +0.0, positive and negative, also for the order edge ownership uses when the own message is the
first in check order (o1 + own where the reference adds own + o1).  A prior of -0.0 DOES show a difference -- the case documents why the rule is
limited to clean inputs (inputs_clean refuses such a prior; the damped and the NaN-tolerant forms keep the add).

The bare loop's alpha prefetch (index min(it + 1, max_iter - 1)) has no test here or on the GPU: what that loop computes is no output."""
import itertools

import numpy as np


def words(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def messages():
    rng = np.random.default_rng(20261021)
    r = rng.standard_normal(6) * np.exp2(rng.integers(-40, 40, 6).astype(np.float64))
    eighths = np.array([0.125, -0.125, 0.375, -2.5, 20.0, -20.0])
    return np.concatenate([[0.0, -0.0], r, -r[:2], eighths, [5e-324, -5e-324, 1.5e308]])


def sums(prior):
    """-> (with the leading 0.0, without it, own-first order of edge ownership), each [triples, priors]"""
    v = messages()
    a, b, c = (np.array(t) for t in zip(*itertools.product(v, repeat=3)))
    p = np.asarray(prior, np.float64)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        ref = (((0.0 + a) + b) + c)[:, None] + p
        new = ((a + b) + c)[:, None] + p
        own_first = ((b + a) + c)[:, None] + p          # check order (a, b, c) with a the own message: the kernel adds o1 = b first
    return ref, new, own_first


def test_the_posterior_word_is_the_same_without_the_leading_zero():
    priors = np.array([0.0, 3.4760986898352733, 1e-310, 27.0, -1.5, -5e-324, -20.0])
    assert not np.signbit(priors[0])
    ref, new, own_first = sums(priors)
    assert ref.shape[0] == len(messages()) ** 3 and np.isfinite(ref).any()
    assert np.array_equal(words(ref), words(new))
    assert np.array_equal(words(ref), words(own_first))
    assert not np.signbit(ref[ref == 0.0]).any()                                # and no posterior is -0.0, which the sign argument of the clean forms needs


def test_a_prior_of_minus_zero_is_why_the_rule_needs_clean_inputs():
    ref, new, _ = sums(np.array([-0.0]))
    differ = words(ref) != words(new)
    v = messages()
    all_minus_zero = np.array([all(x == 0.0 and np.signbit(x) for x in t) for t in itertools.product(v, repeat=3)])
    assert differ.any() and np.array_equal(differ[:, 0], all_minus_zero)        # exactly the triple (-0.0, -0.0, -0.0): +0.0 against -0.0
    assert not np.signbit(ref[differ]).any() and np.signbit(new[differ]).all()
