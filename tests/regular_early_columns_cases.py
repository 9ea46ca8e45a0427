"""Seeded inputs for the passes a shot of the fixed-work ownership form runs before its workgroup reaches the bare loop (csrc/minsum_regular.hip, PLACE):
the syndrome, passes 0 and 1, the freeze and its logical comparison.  The Monte-Carlo form reads the columns of a thread's check in front of the sampler
and keeps the two owned ones, packed, for the freeze; tests/test_regular_early_columns_cpu.py proves with the oracle alone that the inputs have the
properties they are named for, tests/test_regular_early_columns_gpu.py runs them.  Plain module (no pytest hooks); deterministic from the seed below.

Decode API (the form that shares the loop but not the early loads): a NON-uniform clean prior, so pass 0 is the general form, and 20 S syndromes per
graph, ordered so that the first workgroup of every batch holds, side by side, the four ways a shot can leave the kernel:
    shot 0   an unrealisable syndrome: never converges, frozen at it == max_iter (the workgroup never enters the bare loop)
    shot 1   converges at iteration 0: frozen by pass 1
    shot 2   converges at iteration 1: frozen by pass 2
    shot 3   converges at iteration 2: frozen one pass later (at max_iter 2 this one does not converge)
The shots are picked from a seeded pool by what the oracle says about them at max_iter 50; classes() reads the classes of a batch back from the oracle's
outputs at the max_iter under test, and the tests assert them.  The rest of the pool follows in its seeded order: workgroups of every mixture."""
import numpy as np

import regular_shapes as RS

SEED = 20261021
SHAPES = {"bb72": 14, "bb144": 7}                                   # graph -> S
ITERS = (1, 2, 3, 4, 50)
LOW, HIGH = 0.005, 0.05                                             # Monte-Carlo rates: every workgroup leaves through the bare loop / some never enter it
POOL_RATES = (0.01, 0.03, 0.06)                                     # error rates behind the pool's syndromes, shot k takes rate k mod 3
PRIOR_RATES = (0.02, 0.04)                                          # the prior's per-column rates are drawn between these
_CODES, _DECODE = {}, {}


def counts(S):
    """a team without a shot, a workgroup that holds one shot, a last workgroup of two, and twenty workgroups"""
    return (S - 1, S + 1, 3 * S + 2, 20 * S)


def code(name):
    if name not in _CODES:
        from qldpc_amd.data import load_code
        c = load_code(name)
        ip, ix, m, n = c["Hx_indptr"], c["Hx_indices"], int(c["m"]), int(c["n"])
        S = RS.plan(6, m, n)[1]
        assert S == SHAPES[name], (name, S)
        _CODES[name] = (ip, ix, m, n, S, c["Lx"])
    return _CODES[name]


def decode_inputs(name, oracle):
    """-> (prior, syndromes int8[20 S, m]): the four classes first (module docstring), then the rest of the pool"""
    if name not in _DECODE:
        ip, ix, m, n, S, _ = code(name)
        rng = np.random.default_rng([SEED, m])
        q = rng.uniform(PRIOR_RATES[0], PRIOR_RATES[1], n)
        prior = np.log((1 - q) / q)
        B = 20 * S
        rates = np.array(POOL_RATES)[np.arange(B) % len(POOL_RATES)]
        errs = (rng.random((B, n)) < rates[:, None]).astype(np.int64)
        synd = (errs[:, ix.reshape(m, 6)].sum(axis=-1) & 1).astype(np.int8)
        synd[0] = rng.random(m) < 0.5                                                  # unrealisable
        _, conv, _, iters = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=50, threads=0)
        conv, iters = np.asarray(conv).astype(bool), np.asarray(iters)
        assert not conv[0], name
        first = [0] + [int(np.flatnonzero(conv & (iters == k))[0]) for k in (0, 1, 2)]  # IndexError: the pool lacks a class
        order = first + [k for k in range(B) if k not in first]
        _DECODE[name] = (prior, np.ascontiguousarray(synd[order]))
    return _DECODE[name]


def classes(conv, iters):
    """the classes of a batch, from the oracle's outputs -> set of 'never', 'at 0', 'at 1', 'later'"""
    conv, iters = np.asarray(conv).astype(bool), np.asarray(iters)
    out = set()
    if (~conv).any():
        out.add("never")
    for k, what in ((0, "at 0"), (1, "at 1")):
        if (conv & (iters == k)).any():
            out.add(what)
    if (conv & (iters >= 2)).any():
        out.add("later")
    return out


def expected_classes(max_iter):
    """what the first four shots must show at this max_iter: iteration k can only be reached with max_iter > k"""
    return {"never", "at 0"} | ({"at 1"} if max_iter >= 2 else set()) | ({"later"} if max_iter >= 3 else set())
