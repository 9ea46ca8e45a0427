"""The LDS placement of the regular (6,3) min-sum kernel's ownership form (csrc/regular_place.h), no GPU.  tests/regular_place_main.cpp is compiled once
with the compiler the library is built with and prints, per graph and workgroup shape, the ownership table, today's addresses as a table and the placed
table with what the bank model charges each.  Checked here, from the CSR and in Python, independently of the header: every address lies in the R and V
regions and no two items share one; the word the owner of a column reads as its lower and its higher other message is the word those checks store for
that column; the posterior a check gathers for an edge is the one the column's owner stores; a check's gather order and its message-store order name the
same edges, its four stored ones; the lanes of no team have places of their own; the eight gathers and the four message stores are conflict-free by an
independent restatement of the bank model; the posterior stores stay within the cap; the same input gives the same bytes twice; shapes whose arrays do
not fit answer "none"; and today's addresses as a table are today's addresses (the gather cost equals regular_own_cost)."""
import os
import subprocess

import numpy as np
import pytest

import regular_shapes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
RST, OWN_WORDS, WORDS = 7, 16, 16
BB_TAGS = ("bb72", "bb144", "bb288", "bb90", "bb108")
RS_GRAPHS = tuple(name for name, row in RS.TABLE.items() if row[:2] == (6, 3))
FORCED_S = (0, 1, 4)                                            # 0: the plan's own S
CAP_GRAPHS, CAP = ("bb72_Hx", "bb144_Hx", "bb288_Hx"), 2       # posterior-store cycles above 6 per instruction, per workgroup


def all_graphs():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    out = {}
    for tag in BB_TAGS:
        c = load_code(tag)
        out[f"{tag}_Hx"] = (int(c["Hx"].shape[0]), int(c["Hx"].shape[1]), np.asarray(c["Hx_indptr"]), np.asarray(c["Hx_indices"]))
    for name in RS_GRAPHS:
        g = RS.graph(name)
        out[name] = (g.m, g.n, np.asarray(g.indptr), np.asarray(g.indices))
    return out


def text_of(graphs):
    return "".join("%d %d %d\n%s\n%s\n" % (m, n, RST, " ".join(map(str, ip)), " ".join(map(str, ix))) for m, n, ip, ix in graphs)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("regular_place") / "regular_place_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(HERE, "regular_place_main.cpp"), "-o", exe], check=True)

    def run(graphs, force_s=0, max_iter=0):
        return subprocess.run([exe, str(force_s), str(max_iter)], input=text_of(graphs), capture_output=True, text=True, check=True).stdout
    return run


COST_KEYS = ("gather", "post_store", "post_over6", "msg_store", "msg_over6")


def parse(out, graphs):
    """stdout of regular_place_main -> [None or dict(S, TS, block, offV, offD, span, placed, linear, own_cost, cost, own [m, 16], lin [block, 16], rec)]"""
    lines, res, at = out.splitlines(), [], 0

    def cost(ln, tag):
        w = ln.split()
        assert w[0] == tag and len(w) == 1 + 5 + 14
        return dict(zip(COST_KEYS, map(int, w[1:6])), streams=[int(x) for x in w[6:]])

    def table(rows, words):
        nonlocal at
        t = np.array([ln.split() for ln in lines[at:at + rows]], np.int64).reshape(rows, words)
        at += rows
        return t
    for m, *_ in graphs:
        if lines[at] == "none":
            res.append(None)
            at += 1
            continue
        head = lines[at].split()
        assert head[0] == "ok"
        r = dict(zip(("S", "TS", "block", "offV", "offD", "span", "placed"), map(int, head[1:])))
        r["linear"] = cost(lines[at + 1], "linear")
        assert lines[at + 2].split()[0] == "own_cost"
        r["own_cost"] = int(lines[at + 2].split()[1])
        at += 3
        r["cost"] = None
        if r["placed"]:
            r["cost"] = cost(lines[at], "placed")
            at += 1
        r["own"], r["lin"] = table(m, OWN_WORDS), table(r["block"], WORDS)
        r["rec"] = table(r["block"], WORDS) if r["placed"] else None
        res.append(r)
    assert at == len(lines)
    return res


@pytest.fixture(scope="module")
def tables(program):
    """{(name, forced S): (graph, record of parse)} and the raw outputs"""
    G = all_graphs()
    out, raw = {}, {}
    for fs in FORCED_S:
        raw[fs] = program(list(G.values()), fs)
        for (name, g), r in zip(G.items(), parse(raw[fs], list(G.values()))):
            out[name, fs] = (g, r)
    return out, raw


def placed_tables(tables):
    return {k: v for k, v in tables[0].items() if v[1] is not None and v[1]["placed"]}


def test_the_graph_set_and_which_shapes_are_placed(tables):
    T, _ = tables
    assert {"r63_m36", "r63_m257", "r63_m512", "r63_m513"} <= set(RS_GRAPHS)
    for fs in FORCED_S:
        assert T["r63_m513", fs][1] is None                                        # no plan: more checks than a workgroup has threads
    some_none = 0
    for (name, fs), ((m, n, *_), r) in T.items():
        if r is None:
            continue
        assert r["TS"] == m and r["block"] == (r["S"] * m + 63) // 64 * 64 and r["span"] == r["S"] * m * (RST + 2) * 8, (name, fs)
        if fs and m * fs <= RS.LB_T:
            assert r["S"] <= fs, (name, fs)
        fits = 6 * r["block"] * 8 <= r["span"]                                     # 4 * block doubles of messages, 2 * block of posteriors
        assert bool(r["placed"]) == fits, (name, fs, r["block"], r["span"])
        some_none += not fits
    assert some_none >= 2 and not T["bb72_Hx", 1][1]["placed"] and not T["r63_m36", 1][1]["placed"]
    for tag in BB_TAGS:
        assert T[f"{tag}_Hx", 0][1]["placed"] and T[f"{tag}_Hx", 4][1]["placed"], tag
    assert T["r63_m257", 0][1]["placed"] and T["r63_m257", 0][1]["block"] - 257 == 63      # 63 lanes of no team
    assert {1, 4, 7, 14} <= {r["S"] for _, r in placed_tables(tables).values()}


def rows_of_columns(m, n, ip, ix):
    rows = [[] for _ in range(n)]
    for i in range(m):
        for c in ix[ip[i]:ip[i + 1]]:
            rows[int(c)].append(i)
    return rows


def assert_table_is_consistent(key, graph, r, rec, linear):
    """the wiring of a table, from the CSR and the list of who owns which column (words 0 and 1 of the ownership records) alone"""
    m, n, ip, ix = graph
    S, block, own = r["S"], r["block"], r["own"]
    assert sorted(own[:, 0:2].ravel().tolist()) == list(range(n)), key              # every column has one owner
    owner = {int(own[i, v]): (i, v) for i in range(m) for v in range(2)}
    rows = rows_of_columns(m, n, ip, ix)
    hi = (r["offD"] + (RST + 3) * 8) // 8 if linear else r["span"] // 8
    assert rec.shape == (block, WORDS) and (rec[:, 0:14] >= 0).all() and (rec[:, 0:14] < hi).all() and (rec[:, 15] == 0).all(), key
    team = S * m
    if not linear:
        assert (rec[:, 0:14] < r["span"] // 8).all(), key                           # inside R and V
        # items are pairwise distinct: 4 messages and 2 posteriors per lane, the lanes of no team included
        stores = rec[:, 8:14].ravel()
        assert len(set(stores.tolist())) == 6 * block, key
        assert set(rec[:, 0:8].ravel().tolist()) == set(stores.tolist()), key       # whatever is gathered is stored by somebody
        assert set(rec[:, 10:14].ravel().tolist()).isdisjoint(rec[:, 8:10].ravel().tolist()), key
        for t in range(team, block):                                                # a lane of no team reads what it writes, nobody else does
            assert rec[t, 14] == 0, key
            assert set(rec[t, 0:4].tolist()) == set(rec[t, 8:10].tolist()) and set(rec[t, 4:8].tolist()) == set(rec[t, 10:14].tolist()), (key, t)
        assert set(rec[team:, 8:14].ravel().tolist()).isdisjoint(rec[:team, 0:8].ravel().tolist()), key
    for s in range(S):
        base = s * m
        where_post = {int(rec[base + o, 8 + v]): int(own[o, v]) for o in range(m) for v in range(2)}      # address -> the column whose posterior lives there
        assert len(where_post) == n, (key, s)
        stored_for = {}                                                             # (check, column) -> where the check stores its message for the column
        for i in range(m):
            csr = [int(c) for c in ix[ip[i]:ip[i + 1]]]
            others = [c for c in csr if owner[c][0] != i]
            assert len(others) == 4 and sorted(int(own[i, v]) for v in range(2)) == sorted(set(csr) - set(others)), (key, i)
            cols = [where_post[int(a)] for a in rec[base + i, 0:4]]                 # the gather order: edge 2 + k of the kernel is the column gathered k-th
            assert sorted(cols) == sorted(others), (key, s, i)                      # the four stored edges, each once, gathered where their owner stores
            named = [int(own[i, (int(rec[base + i, 14]) >> (4 * k)) & 15]) for k in range(4)]
            assert named == cols, (key, s, i)                                       # word 14 says the same
            for k in range(4):
                stored_for[i, cols[k]] = int(rec[base + i, 10 + k])                 # the message store of edge 2 + k: the same order by construction of the kernel
        assert len(set(stored_for.values())) == 4 * m, (key, s)
        for i in range(m):
            for v in range(2):
                j = int(own[i, v])
                lo, hi_ = [x for x in rows[j] if x != i]
                assert lo < hi_ and int(rec[base + i, 4 + 2 * v]) == stored_for[lo, j] and int(rec[base + i, 5 + 2 * v]) == stored_for[hi_, j], (key, s, i, v)


def test_every_placed_table_is_wired_as_the_graph_says(tables):
    seen = 0
    for key, (g, r) in placed_tables(tables).items():
        assert_table_is_consistent(key, g, r, r["rec"], linear=False)
        seen += 1
    assert seen >= 20


def test_todays_addresses_as_a_table_are_todays_addresses(tables):
    T, _ = tables
    for key, ((m, n, ip, ix), r) in T.items():
        if r is None:
            continue
        assert_table_is_consistent(key, (m, n, ip, ix), r, r["lin"], linear=True)
        lin, S = r["lin"], r["S"]
        for s in range(S):
            i = np.arange(m)
            t = s * m + i
            assert (lin[t, 0:4] == r["offV"] // 8 + s * n + r["own"][:, 6:10]).all() and (lin[t, 4:8] == s * m * RST + r["own"][:, 10:14]).all(), key
            assert (lin[t, 8] == r["offV"] // 8 + s * n + i).all() and (lin[t, 9] == r["offV"] // 8 + s * n + i + m).all(), key
            assert (lin[t, 10:14] == ((s * m + i) * RST)[:, None] + np.arange(4)).all(), key
        d = r["offD"] // 8
        for t in range(S * m, r["block"]):
            assert lin[t, 0:14].tolist() == [d + RST, d + RST + 1, d + RST, d + RST + 1, d, d + 1, d, d + 1, d + RST, d + RST + 1, d, d + 1, d + 2, d + 3], key
        if key[1] == 0 and m <= RS.LB_T:
            assert r["linear"]["gather"] == r["own_cost"], key                     # the same rule as regular_own_cost, on the same addresses


# ---------------------------------------------------------------------------------------- the bank model, restated
def model(rec, block):
    """ds_read_b64: 32-lane groups, pair-bank = address mod 32; ds_write_b64: 16-lane groups, bank = address mod 16; a group costs the largest number of
    distinct addresses on one bank, a wave-instruction the sum of its groups -> (per-stream cycles [14], per-stream cycles above 6 per instruction [14])"""
    cyc, over = [0] * 14, [0] * 14
    for w in range(14):
        lanes = 32 if w < 8 else 16
        for t0 in range(0, block, 64):
            c = 0
            for g0 in range(t0, t0 + 64, lanes):
                banks = {}
                for a in rec[g0:g0 + lanes, w].tolist():
                    banks.setdefault(a % lanes, set()).add(a)
                c += max(len(v) for v in banks.values())
            cyc[w] += c
            over[w] += max(0, c - 6)
    return cyc, over


def test_the_gathers_and_the_message_stores_are_conflict_free(tables):
    for key, (g, r) in placed_tables(tables).items():
        block, c = r["block"], r["cost"]
        cyc, over = model(r["rec"], block)
        assert cyc == c["streams"], key                                            # the header's model and this one agree stream by stream
        assert c["gather"] == sum(cyc[0:8]) == 8 * (block // 32), key
        assert cyc[0:8] == [block // 32] * 8, key
        assert c["msg_store"] == sum(cyc[10:14]) == 4 * (block // 16) and c["msg_over6"] == sum(over[10:14]) == 0, key
        assert c["post_store"] == sum(cyc[8:10]) and c["post_over6"] == sum(over[8:10]), key
        assert c["post_store"] >= 2 * (block // 16), key
        lc, lo = model(r["lin"], block)
        assert lc == r["linear"]["streams"] and sum(lo[8:10]) == r["linear"]["post_over6"], key
        print(f"{key[0]} S {r['S']} block {block}: gathers {r['linear']['gather']} -> {c['gather']}, message stores {r['linear']['msg_store']} -> {c['msg_store']}, "
              f"posterior stores {r['linear']['post_store']} -> {c['post_store']} (free {2 * (block // 16)}), above 6 per instruction {c['post_over6']}")


def test_the_posterior_stores_stay_within_the_cap(tables):
    T, _ = tables
    for name in CAP_GRAPHS:
        for fs in FORCED_S:
            r = T[name, fs][1]
            if r["placed"]:
                assert r["cost"]["post_over6"] <= CAP, (name, fs, r["cost"])
        assert T[name, 0][1]["placed"], name


def test_two_runs_give_identical_bytes(program, tables):
    _, raw = tables
    G = all_graphs()
    for fs in FORCED_S:
        assert program(list(G.values()), fs) == raw[fs]


def test_a_large_iteration_table_changes_the_shape_and_the_table(program):
    """max_iter enters the carve (alpha lives behind V), so S can fall: the placement is per (S, block), not per graph"""
    G = all_graphs()
    g = G["bb144_Hx"]
    a, b = parse(program([g], 0, 0), [g])[0], parse(program([g], 0, 1024), [g])[0]
    assert a["S"] == 7 and b["S"] < a["S"] and b["placed"]
    assert_table_is_consistent(("bb144_Hx", "max_iter 1024"), g, b, b["rec"], linear=False)
    assert model(b["rec"], b["block"])[0][0:8] == [b["block"] // 32] * 8
