"""Edge ownership of the regular (6,3) min-sum kernel (csrc/regular_own.h: pure C++, no HIP header), no GPU: a stand-alone host program
(tests/regular_own_main.cpp) is compiled once with the compiler the library is built with and prints the per-check records for every graph below.
The records are held against the CSR, and a numpy model of one pass that keeps two edges of each check inside its thread -- the check update restated
in the kernel's compare-free form, the variable sum as ((0.0 + o1) + X) + Y with (X, Y) = last ? (o2, own) : (own, o2) -- is held word for word
against the plain pass in the reference's order (first strict minimum gets min2, ascending-check-order sums)."""
import os
import subprocess

import numpy as np
import pytest

import regular_shapes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
RST, WORDS = 7, 16
BB_TAGS = ("bb72", "bb144", "bb288", "bb90", "bb108")
RS_GRAPHS = tuple(name for name, row in RS.TABLE.items() if row[:2] == (6, 3))


def all_graphs():
    """-> {name: (m, n, indptr, indices)}: both sectors of the BB codes and every (6,3) graph of regular_shapes (m = 513 included: the header has no
    team-size limit, the plan has)"""
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    out = {}
    for tag in BB_TAGS:
        c = load_code(tag)
        for h in ("Hx", "Hz"):
            out[f"{tag}_{h}"] = (int(c[h].shape[0]), int(c[h].shape[1]), np.asarray(c[h + "_indptr"]), np.asarray(c[h + "_indices"]))
    for name in RS_GRAPHS:
        g = RS.graph(name)
        out[name] = (g.m, g.n, np.asarray(g.indptr), np.asarray(g.indices))
    return out


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("regular_own") / "regular_own_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "regular_own_main.cpp"), "-o", exe], check=True)

    def ask(graphs):
        """[(m, n, indptr, indices)] -> [int array [m, 16] or None]"""
        text = "".join("%d %d %d\n%s\n%s\n" % (m, n, RST, " ".join(map(str, ip)), " ".join(map(str, ix))) for m, n, ip, ix in graphs)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        out, at = [], 0
        for m, *_ in graphs:
            if lines[at] == "none":
                out.append(None)
                at += 1
            else:
                assert lines[at] == "ok"
                out.append(np.array([[int(x) for x in ln.split()] for ln in lines[at + 1:at + 1 + m]], np.int64).reshape(m, WORDS))
                at += 1 + m
        assert at == len(lines)
        return out
    return ask


@pytest.fixture(scope="module")
def tables(records):
    G = all_graphs()
    return {name: (g, T) for (name, g), T in zip(G.items(), records(list(G.values())))}


def rows_of_columns(m, n, ip, ix):
    rows = [[] for _ in range(n)]
    for i in range(m):
        for c in ix[ip[i]:ip[i + 1]]:
            rows[c].append(i)
    return rows


def test_graph_set(tables):
    assert len(tables) == 2 * len(BB_TAGS) + len(RS_GRAPHS) and {"r63_m36", "r63_m257", "r63_m513"} <= set(RS_GRAPHS)
    for name, (g, T) in tables.items():
        assert T is not None and T.shape == (g[0], WORDS), name


def test_every_column_has_one_adjacent_owner_and_every_check_owns_two(tables):
    for name, ((m, n, ip, ix), T) in tables.items():
        owned = T[:, 0:2]
        assert sorted(owned.ravel().tolist()) == list(range(n)), name                      # every column once
        for i in range(m):
            csr = ix[ip[i]:ip[i + 1]].tolist()
            assert sorted(T[i, 0:6].tolist()) == sorted(csr), (name, i)                    # the six columns of the check, reordered
            assert T[i, 0] < T[i, 1], (name, i)                                            # two distinct owned columns, both of this check
            assert T[i, 2:6].tolist() == [c for c in csr if c not in (T[i, 0], T[i, 1])], (name, i)      # the stored ones keep CSR order
            assert T[i, 15] == 0 and 0 <= T[i, 14] < 4


def test_last_and_other_messages_follow_ascending_check_order(tables):
    seen_positions = set()
    for name, ((m, n, ip, ix), T) in tables.items():
        rows = rows_of_columns(m, n, ip, ix)
        for i in range(m):
            for v in range(2):
                r = rows[T[i, v]]
                assert r == sorted(r) and len(r) == 3 and i in r
                others = [x for x in r if x != i]
                o1, o2 = T[i, 10 + 2 * v], T[i, 11 + 2 * v]
                assert [o1 // RST, o2 // RST] == others, (name, i, v)
                assert bool((T[i, 14] >> v) & 1) == (i == r[2]), (name, i, v)
                seen_positions.add(r.index(i))
    assert seen_positions == {0, 1, 2}


def test_stored_slots_and_read_offsets_name_the_same_words(tables):
    for name, ((m, n, ip, ix), T) in tables.items():
        place = {int(T[i, v]): i + m * v for i in range(m) for v in range(2)}              # a thread keeps its posteriors at V[i] and V[i + m]
        assert (T[:, 6:10] == np.vectorize(place.get)(T[:, 2:6])).all(), name              # and the four gathers of a check read those places
        written = {}                                                                       # word -> column whose message it holds
        for i in range(m):
            for k in range(4):
                w = i * RST + k                                                            # the kernel stores edge k at slot k - 2
                assert w not in written
                written[w] = T[i, 2 + k]
        read = {}
        for i in range(m):
            for v in range(2):
                for w in T[i, 10 + 2 * v:12 + 2 * v]:
                    assert 0 <= w < m * RST and w not in read
                    read[int(w)] = T[i, v]
        assert read == written and len(read) == 4 * m, name                                # every stored word is read once, as a message of its column


def test_a_repeated_column_in_a_row_gives_none(tables, records):
    (m, n, ip, ix), _ = tables["bb72_Hx"]
    ix = ix.copy()
    row = lambda i: ix[ip[i]:ip[i + 1]]          # noqa: E731
    # row 0 trades its column c for a second copy of its column a; a row u that has a and not c trades a for c: every degree stays what it was
    a, c = row(0)[0], row(0)[1]
    u = next(i for i in range(1, m) if a in row(i) and c not in row(i))
    row(0)[1] = a
    row(u)[np.flatnonzero(row(u) == a)[0]] = c
    assert np.bincount(ix, minlength=n).tolist() == [3] * n
    short = (m - 1, n, ip[:-1], ix[:ip[m - 1]])                                            # and a graph that is not (6,3) at all
    assert records([(m, n, ip, ix), short, tables["bb72_Hx"][0]])[:2] == [None, None]


# ---------------------------------------------------------------------------------------- one pass, word for word
def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def plain_pass(cols, rows, pos, V, Rprev, syn, alpha, clip, prior):
    """the reference's pass on CSR order: (messages [m, 6], posteriors [n])"""
    t = np.clip(V[cols] - Rprev, -clip, clip)
    neg = t < 0.0                                                          # -0.0 counts as >= 0
    a = np.abs(t)
    order = np.argsort(a, axis=1, kind="stable")                           # the first strict minimum comes first
    ar = np.arange(len(cols))
    min1, min2, first = a[ar, order[:, 0]], a[ar, order[:, 1]], order[:, 0]
    mag = np.where(np.arange(6)[None, :] == first[:, None], min2[:, None], min1[:, None])
    sgn = (syn[:, None] ^ np.bitwise_xor.reduce(neg, axis=1)[:, None]) ^ neg
    msg = (alpha * np.where(sgn, -1.0, 1.0)) * mag
    out = np.empty_like(V)
    for j in range(len(V)):
        s = np.float64(0.0)
        for r, p in zip(rows[j], pos[j]):                                  # ascending check order
            s = s + msg[r, p]
        out[j] = s + prior[j]
    return msg, out


def owned_pass(T, V, Rprev_re, syn, alpha, clip, prior):
    """the kernel's pass: reordered rows, compare-free check update, four stored words per check, owned variable sums
    -> (messages in reordered order [m, 6], posteriors [n])"""
    m = len(T)
    reg = np.stack([V[T[:, 0]], V[T[:, 1]]], axis=1)                       # the two owned posteriors, in registers
    Vl = np.concatenate([reg[:, 0], reg[:, 1]])                            # and in LDS at V[i], V[i + m]
    t = np.concatenate([reg, Vl[T[:, 6:10]]], axis=1) - Rprev_re
    sb = np.signbit(t)
    spw = syn ^ np.bitwise_xor.reduce(sb, axis=1)
    a = np.abs(t)
    suf = np.empty_like(a)
    suf[:, 5] = np.minimum(a[:, 5], clip)
    for k in range(4, 0, -1):
        suf[:, k] = np.minimum(a[:, k], suf[:, k + 1])
    msg = np.empty_like(a)
    pre = None
    for k in range(6):
        mag = suf[:, 1] if k == 0 else pre if k == 5 else np.minimum(pre, suf[:, k + 1])
        if k < 5:
            pre = np.minimum(a[:, 0], clip) if k == 0 else np.minimum(a[:, k], pre)
        msg[:, k] = np.copysign(alpha * mag, np.where(spw ^ sb[:, k], -1.0, 1.0))
    R = np.full(m * RST, np.nan)                                           # LDS rows: a word nobody stored stays NaN
    for k in range(4):
        R[np.arange(m) * RST + k] = msg[:, 2 + k]
    out = np.full(len(V), np.nan)
    for v in range(2):
        o1, o2, own = R[T[:, 10 + 2 * v]], R[T[:, 11 + 2 * v]], msg[:, v]
        last = ((T[:, 14] >> v) & 1).astype(bool)
        s = ((np.float64(0.0) + o1) + np.where(last, o2, own)) + np.where(last, own, o2)
        out[T[:, v]] = s + prior[T[:, v]]
    return msg, out


@pytest.mark.parametrize("kind", ["normal", "dyadic"])
def test_one_pass_equals_the_plain_pass_word_for_word(tables, kind):
    """normal: random doubles, so that a sum in another order rounds to another word.  dyadic: multiples of 1/8, so that t == 0 (messages of magnitude
    0, of either sign: +-0.0), tied minima and exact cancellations are common."""
    saw_negzero = saw_tie = False
    for name in ("bb72_Hx", "bb144_Hz", "bb90_Hx", "r63_m36", "r63_m257"):
        (m, n, ip, ix), T = tables[name]
        cols = ix.reshape(m, 6).astype(np.int64)
        rows = rows_of_columns(m, n, ip, ix)
        pos = [[cols[r].tolist().index(j) for r in rows[j]] for j in range(n)]
        perm = np.array([[cols[i].tolist().index(c) for c in T[i, 0:6]] for i in range(m)])       # reordered edge k = CSR edge perm[i, k]
        for trial in range(6):
            rng = np.random.default_rng([20261019, m, trial, kind == "dyadic"])
            if kind == "normal":
                V, Rprev, prior = rng.normal(0, 3, n), rng.normal(0, 2, (m, 6)), rng.normal(2, 1, n)
                alpha, clip = 0.8371, 2.5
            else:
                V, Rprev, prior = rng.integers(-12, 13, n) / 8.0, rng.integers(-12, 13, (m, 6)) / 8.0, rng.integers(-8, 9, n) / 8.0
                V = V + 0.0                                                # a posterior is never -0.0 (csrc/minsum_regular.hip, header comment)
                Rprev[rng.random((m, 6)) < 0.05] = -0.0                    # a message may be
                alpha, clip = 0.75, 1.0
            syn = rng.random(m) < 0.3
            ref_msg, ref_V = plain_pass(cols, rows, pos, V, Rprev, syn, alpha, clip, prior)
            got_msg, got_V = owned_pass(T, V, Rprev[np.arange(m)[:, None], perm], syn, alpha, clip, prior)
            assert np.array_equal(bits(got_msg), bits(ref_msg[np.arange(m)[:, None], perm])), (name, trial)
            assert np.array_equal(bits(got_V), bits(ref_V)), (name, trial)
            saw_negzero |= bool((np.signbit(ref_msg) & (ref_msg == 0)).any())
            a = np.sort(np.abs(np.clip(V[cols] - Rprev, -clip, clip)), axis=1)
            saw_tie |= bool((a[:, 0] == a[:, 1]).any())
    if kind == "dyadic":
        assert saw_negzero and saw_tie
