"""The choice among edge-ownership assignments of the regular (6,3) min-sum kernel (csrc/regular_own.h: regular_own_cost, regular_own_assign with
search), no GPU.  Two stand-alone host programs are compiled once with the compiler the library is built with: tests/regular_own_main.cpp prints the
records the library would upload, tests/regular_own_cost_main.cpp the kind of the chosen candidate, the bank-model cost of the assignment without
search and of the chosen one, and the chosen records.  Checked here: the chosen tables have every property the kernel relies on (restated, not
imported), a numpy model of one pass on them equals the plain pass word for word, the cost never exceeds that of the first matching and falls to
three quarters of it or less on the Hx matrices of bb72 / bb144 / bb288, the translation-invariant candidates are found exactly on the
bivariate-bicycle matrices, the output is the same bytes on every run, and an independent restatement of the bank model agrees on every table."""
import os
import subprocess

import numpy as np
import pytest

import regular_shapes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
RST, WORDS, LB_T = 7, 16, 512
BB_TAGS = ("bb72", "bb144", "bb288", "bb90", "bb108")
RS_GRAPHS = tuple(name for name, row in RS.TABLE.items() if row[:2] == (6, 3))
RATIO_GRAPHS, RATIO = ("bb72_Hx", "bb144_Hx", "bb288_Hx"), 0.75


def all_graphs():
    """-> {name: (m, n, indptr, indices)}: both sectors of the BB codes and every (6,3) graph of regular_shapes"""
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


def relabelled(graph, seed):
    """the same graph with its checks in a random order (columns, and the order of a row's columns, as they were)"""
    m, n, ip, ix = graph
    perm = np.random.default_rng(seed).permutation(m)
    return m, n, ip.copy(), ix.reshape(m, 6)[perm].ravel().copy()


def text_of(graphs):
    return "".join("%d %d %d\n%s\n%s\n" % (m, n, RST, " ".join(map(str, ip)), " ".join(map(str, ix))) for m, n, ip, ix in graphs)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """-> (own(graphs) -> raw stdout of regular_own_main, cost(graphs, search = 1) -> raw stdout of regular_own_cost_main)"""
    d = tmp_path_factory.mktemp("regular_own_search")
    exes = {}
    for name in ("regular_own_main", "regular_own_cost_main"):
        exes[name] = str(d / name)
        subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, name + ".cpp"), "-o", exes[name]], check=True)

    def own(graphs):
        return subprocess.run([exes["regular_own_main"]], input=text_of(graphs), capture_output=True, text=True, check=True).stdout

    def cost(graphs, search=1):
        return subprocess.run([exes["regular_own_cost_main"], str(search)], input=text_of(graphs), capture_output=True, text=True, check=True).stdout
    return own, cost


def parse_cost(out, graphs):
    """stdout of regular_own_cost_main -> [None or dict(kind, L, M, candidates, S, TS, block, offV, offD, kuhn, kuhn_streams, cost, streams, T [m, 16])]"""
    lines, res, at = out.splitlines(), [], 0
    for m, *_ in graphs:
        if lines[at] == "none":
            res.append(None)
            at += 1
            continue
        head, kuhn, chosen = lines[at].split(), lines[at + 1].split(), lines[at + 2].split()
        assert head[0] == "ok" and kuhn[0] == "kuhn" and chosen[0] == "chosen" and len(kuhn) == len(chosen) == 10
        r = dict(zip(("L", "M", "candidates", "S", "TS", "block", "offV", "offD"), map(int, head[2:])), kind=head[1])
        r.update(kuhn=int(kuhn[1]), kuhn_streams=[int(x) for x in kuhn[2:]], cost=int(chosen[1]), streams=[int(x) for x in chosen[2:]])
        r["T"] = np.array([[int(x) for x in ln.split()] for ln in lines[at + 3:at + 3 + m]], np.int64).reshape(m, WORDS)
        res.append(r)
        at += 3 + m
    assert at == len(lines)
    return res


@pytest.fixture(scope="module")
def chosen(programs):
    """{name: (graph, record of parse_cost)} with search, and the raw outputs for the byte comparisons"""
    G = all_graphs()
    own, cost = programs
    raw = cost(list(G.values()))
    return {name: (g, r) for (name, g), r in zip(G.items(), parse_cost(raw, list(G.values())))}, raw


def rows_of_columns(m, n, ip, ix):
    rows = [[] for _ in range(n)]
    for i in range(m):
        for c in ix[ip[i]:ip[i + 1]]:
            rows[c].append(i)
    return rows


def assert_valid_table(name, graph, T):
    """every property of a table the kernel relies on (csrc/regular_own.h, header comment); -> the positions the own message takes in a column's sum"""
    m, n, ip, ix = graph
    assert T.shape == (m, WORDS), name
    assert sorted(T[:, 0:2].ravel().tolist()) == list(range(n)), name                      # every column has exactly one owner
    rows = rows_of_columns(m, n, ip, ix)
    positions = set()
    for i in range(m):
        csr = ix[ip[i]:ip[i + 1]].tolist()
        assert sorted(T[i, 0:6].tolist()) == sorted(csr), (name, i)                        # the six columns of the check: both owned ones are adjacent to it
        assert T[i, 0] < T[i, 1], (name, i)                                                # two owned, ascending
        assert T[i, 2:6].tolist() == [c for c in csr if c not in (T[i, 0], T[i, 1])], (name, i)      # the stored ones keep CSR order
        assert T[i, 15] == 0 and 0 <= T[i, 14] < 4, (name, i)
        for v in range(2):
            r = rows[T[i, v]]
            assert r == sorted(r) and len(r) == 3 and i in r, (name, i, v)
            assert [T[i, 10 + 2 * v] // RST, T[i, 11 + 2 * v] // RST] == [x for x in r if x != i], (name, i, v)      # o1, o2 in ascending check order
            assert bool((T[i, 14] >> v) & 1) == (i == r[2]), (name, i, v)                  # last
            positions.add(r.index(i))
    place = {int(T[i, v]): i + m * v for i in range(m) for v in range(2)}                  # a thread keeps its posteriors at V[i] and V[i + m]
    assert (T[:, 6:10] == np.vectorize(place.get)(T[:, 2:6])).all(), name
    written = {i * RST + k: int(T[i, 2 + k]) for i in range(m) for k in range(4)}          # the kernel stores edge k at slot k - 2
    read = {}
    for i in range(m):
        for v in range(2):
            for w in T[i, 10 + 2 * v:12 + 2 * v]:
                assert 0 <= w < m * RST and int(w) not in read, (name, i, v)
                read[int(w)] = int(T[i, v])
    assert read == written and len(read) == 4 * m, name                                    # every stored word is read exactly once, as a message of its column
    return positions


def test_graph_set_and_tables_are_valid(chosen):
    tables, _ = chosen
    assert len(tables) == 2 * len(BB_TAGS) + len(RS_GRAPHS) and {"r63_m36", "r63_m257", "r63_m513"} <= set(RS_GRAPHS)
    positions = set()
    for name, (g, r) in tables.items():
        assert r is not None, name
        positions |= assert_valid_table(name, g, r["T"])
    assert positions == {0, 1, 2}                                                          # the own message first, second and third


def test_library_program_prints_the_chosen_table(programs, chosen):
    """regular_own_main calls regular_own_assign as it stands: its records are the chosen ones, and those without search are the first matching's"""
    tables, _ = chosen
    own, cost = programs
    graphs = [g for g, _ in tables.values()]
    lines = own(graphs).splitlines()
    at = 0
    for name, (g, r) in tables.items():
        assert lines[at] == "ok"
        assert np.array_equal(np.array([ln.split() for ln in lines[at + 1:at + 1 + g[0]]], np.int64), r["T"]), name
        at += 1 + g[0]
    for (name, (g, r)), k in zip(tables.items(), parse_cost(cost(graphs, 0), graphs)):
        assert (k["kind"], k["cost"], k["streams"]) == ("kuhn", r["kuhn"], r["kuhn_streams"]) and k["kuhn"] == r["kuhn"], name
        assert_valid_table(name + " without search", g, k["T"])


def test_chosen_cost_against_the_first_matching(chosen):
    tables, _ = chosen
    for name, (g, r) in tables.items():
        print(f"{name}: {r['kind']} S {r['S']} first matching {r['kuhn']} chosen {r['cost']} ratio {r['cost'] / r['kuhn']:.3f}")
        assert r["cost"] <= r["kuhn"], name
        assert r["cost"] == sum(r["streams"]) and r["kuhn"] == sum(r["kuhn_streams"]), name
        assert (r["kind"] == "kuhn") == (r["cost"] == r["kuhn"]), name                     # ties go to the first matching
    for name in RATIO_GRAPHS:
        r = tables[name][1]
        assert r["cost"] <= RATIO * r["kuhn"], (name, r["cost"], r["kuhn"])


def test_cyclic_candidates_are_found_on_the_bb_matrices_only(chosen):
    tables, _ = chosen
    for name, ((m, *_), r) in tables.items():
        if name.startswith("bb"):
            assert r["candidates"] >= 9 and r["candidates"] % 9 == 0 and r["kind"] == "cyclic" and r["L"] * r["M"] == m, (name, r["kind"], r["candidates"])
        else:
            assert r["candidates"] == 0 and r["kind"] == "searched", (name, r["kind"], r["candidates"])


def test_a_relabelled_bb_matrix_takes_the_search(programs, chosen):
    tables, _ = chosen
    own, cost = programs
    graphs = [relabelled(tables[name][0], [20261019, k]) for k, name in enumerate(("bb72_Hx", "bb144_Hx", "bb108_Hz"))]
    for g, r in zip(graphs, parse_cost(cost(graphs), graphs)):
        assert r is not None and r["candidates"] == 0 and r["kind"] in ("searched", "kuhn")
        assert_valid_table("relabelled", g, r["T"])
        assert r["cost"] <= r["kuhn"] and (r["kind"] == "kuhn") == (r["cost"] == r["kuhn"])


def test_two_runs_give_identical_bytes(programs, chosen):
    tables, raw = chosen
    own, cost = programs
    graphs = [g for g, _ in tables.values()]
    assert cost(graphs) == raw
    assert own(graphs) == own(graphs)


def test_a_repeated_column_in_a_row_gives_none(programs, chosen):
    tables, _ = chosen
    own, cost = programs
    m, n, ip, ix = tables["bb72_Hx"][0]
    ix = ix.copy()
    row = lambda i: ix[ip[i]:ip[i + 1]]          # noqa: E731
    # row 0 trades its column c for a second copy of its column a; a row u that has a and not c trades a for c: every degree stays what it was
    a, c = row(0)[0], row(0)[1]
    u = next(i for i in range(1, m) if a in row(i) and c not in row(i))
    row(0)[1] = a
    row(u)[np.flatnonzero(row(u) == a)[0]] = c
    assert np.bincount(ix, minlength=n).tolist() == [3] * n
    graphs = [(m, n, ip, ix), (m - 1, n, ip[:-1], ix[:ip[m - 1]]), tables["bb72_Hx"][0]]   # the second: not (6,3) at all
    got = parse_cost(cost(graphs), graphs)
    assert got[0] is None and got[1] is None and got[2] is not None
    assert own(graphs).splitlines()[:3] == ["none", "none", "ok"]


# ---------------------------------------------------------------------------------------- the bank model, restated
def carve(m):
    """the workgroup the cost is taken at: plan_regular_shape of csrc/regular_plan.h for a (6,3) graph without an iteration table (one alpha word), and one
    team in one workgroup of its own size where the graph has more checks than a workgroup has threads -> (S, block, offV, offD) in bytes"""
    n, nq = 2 * m, (2 * m + 3) // 4

    def offsets(s):
        off_v = s * m * RST * 8
        off_e = off_v + s * n * 8
        off_l = (off_e + s * nq * 4 + 7) // 8 * 8
        off_i = off_l + s * 8
        off_a = (off_i + (6 * s + 2) * 4 + 7) // 8 * 8
        return off_v, off_a + 8 + 6 * 8 + 16
    S = max(LB_T, m) // m
    while S > 1 and offsets(S)[1] > 39 * 1024:
        S -= 1
    return (S, (S * m + 63) // 64 * 64) + offsets(S)


def model_cost(m, T, S, block, off_v, off_d):
    """LDS-array cycles of the eight gathers over one workgroup: ds_read_b64 serves lanes 0..31 and 32..63 of a wave as two groups, a double lives on
    pair-bank (byte address / 8) mod 32, a group costs the largest number of distinct addresses on one pair-bank -> per-stream list"""
    n = 2 * m
    out = []
    for s in range(8):
        total = 0
        for t0 in range(0, block, 32):
            banks = {}
            for t in range(t0, t0 + 32):
                slot, member = divmod(t, m)
                if slot < S:
                    byte = off_v + 8 * (slot * n + int(T[member, 6 + s])) if s < 4 else 8 * (slot * m * RST + int(T[member, 10 + s - 4]))
                else:                                                  # a lane of no team: the dummy row, then two dummy posteriors
                    byte = off_d + 8 * (RST + (s & 1)) if s < 4 else off_d + 8 * (s & 1)
                banks.setdefault((byte // 8) % 32, set()).add(byte)
            total += max(len(v) for v in banks.values())
        out.append(total)
    return out


def test_the_restated_bank_model_agrees_on_every_table(programs, chosen):
    tables, _ = chosen
    own, cost = programs
    graphs = [g for g, _ in tables.values()]
    conflict_free = {"bb72_Hx": 9.14, "bb144_Hx": 18.29, "bb288_Hx": 37.33}               # 2 groups * 8 gathers * waves / S
    for (name, ((m, *_), r)), k in zip(tables.items(), parse_cost(cost(graphs, 0), graphs)):
        S, block, off_v, off_d = carve(m)
        assert (S, m, block, off_v, off_d) == (r["S"], r["TS"], r["block"], r["offV"], r["offD"]), name
        if m <= LB_T:
            assert (m, S, block) == RS.plan(6, m, 2 * m, max_iter=0)[:3], name
        assert model_cost(m, r["T"], S, block, off_v, off_d) == r["streams"], name
        assert model_cost(m, k["T"], S, block, off_v, off_d) == r["kuhn_streams"], name
        assert min(r["streams"]) >= block // 32, name                                      # a group costs at least one cycle
        if name in conflict_free:
            assert round(8 * (block // 32) / S, 2) == conflict_free[name]


# ---------------------------------------------------------------------------------------- one pass, word for word
def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def plain_pass(cols, rows, pos, V, Rprev, syn, alpha, clip, prior):
    """the reference's pass on CSR order: the first strict minimum gets min2, sums in ascending check order -> (messages [m, 6], posteriors [n])"""
    t = np.clip(V[cols] - Rprev, -clip, clip)
    neg = t < 0.0                                                          # -0.0 counts as >= 0
    a = np.abs(t)
    order = np.argsort(a, axis=1, kind="stable")
    ar = np.arange(len(cols))
    min1, min2, first = a[ar, order[:, 0]], a[ar, order[:, 1]], order[:, 0]
    mag = np.where(np.arange(6)[None, :] == first[:, None], min2[:, None], min1[:, None])
    sgn = (syn[:, None] ^ np.bitwise_xor.reduce(neg, axis=1)[:, None]) ^ neg
    msg = (alpha * np.where(sgn, -1.0, 1.0)) * mag
    out = np.empty_like(V)
    for j in range(len(V)):
        s = np.float64(0.0)
        for r, p in zip(rows[j], pos[j]):
            s = s + msg[r, p]
        out[j] = s + prior[j]
    return msg, out


def owned_pass(T, V, Rprev_re, syn, alpha, clip, prior):
    """the kernel's pass on a table: reordered rows, compare-free check update (prefix and suffix minima seeded with the clip), four stored words per
    check, owned sums ((0.0 + o1) + X) + Y with (X, Y) = last ? (o2, own) : (own, o2) -> (messages in reordered order [m, 6], posteriors [n])"""
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
def test_one_pass_on_the_chosen_tables_equals_the_plain_pass_word_for_word(chosen, kind):
    """normal: random doubles, so that a sum in another order rounds to another word.  dyadic: multiples of 1/8, so that t == 0 (messages of magnitude 0
    of either sign: +-0.0), tied minima and exact cancellations are common.  Cyclic and searched tables both."""
    tables, _ = chosen
    saw_negzero = saw_tie = False
    positions = set()
    for name in ("bb72_Hx", "bb144_Hx", "bb288_Hz", "bb90_Hx", "r63_m36", "r63_m257"):
        (m, n, ip, ix), r = tables[name]
        T = r["T"]
        cols = ix.reshape(m, 6).astype(np.int64)
        rows = rows_of_columns(m, n, ip, ix)
        positions |= {rows[T[i, v]].index(i) for i in range(m) for v in range(2)}
        pos = [[cols[x].tolist().index(j) for x in rows[j]] for j in range(n)]
        perm = np.array([[cols[i].tolist().index(c) for c in T[i, 0:6]] for i in range(m)])       # reordered edge k = CSR edge perm[i, k]
        for trial in range(4):
            rng = np.random.default_rng([20261020, m, trial, kind == "dyadic"])
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
    assert positions == {0, 1, 2}
    if kind == "dyadic":
        assert saw_negzero and saw_tie
