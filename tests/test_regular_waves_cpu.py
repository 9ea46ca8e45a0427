"""The class-uniform waves of the regular (6,3) min-sum kernel, no GPU: the min-last ownership assignment (csrc/regular_own.h), the thread order and the
placement under it (csrc/regular_place.h).  tests/regular_waves_main.cpp is compiled once with the compiler the library is built with and prints the
tables; everything is checked here from the CSR, in Python.  Over the Hx matrices of bb72, bb144, bb288, bb90, bb108 and the r63 graphs of
regular_shapes.py, at the plan's own S and with S forced to 1 and 4: the assignment is perfect; it owns as few `last` edges as an independent min-cost
solve (scipy) and, on the five BB matrices, the figures the assignment was specified with; a check owning exactly one last edge holds it as column 1; the
thread map is a bijection onto the block's threads; a wave labelled none, one or both holds only that class among its team lanes; bb144 at S = 7 has at
least 6 select-free waves of 8; the placed table is wired as the graph says and its record names the thread's (slot, member) and its wave's class; the
modelled gathers and message stores are conflict-free; the posterior stores' cycles above 6 per instruction are no worse than those of the bank-model
assignment in the identity order; and the bank-model assignment's words are the ones tests/regular_place_main.cpp prints (the existing table, unchanged
by the second one)."""
import os
import subprocess

import numpy as np
import pytest

import regular_shapes as RS
import test_regular_place_cpu as RP

HERE = os.path.dirname(os.path.abspath(__file__))
RST, WORDS = RP.RST, RP.WORDS
FORCED_S = (0, 1, 4)
MIN_LAST = {"bb72_Hx": 7, "bb144_Hx": 11, "bb288_Hx": 22, "bb90_Hx": 9, "bb108_Hx": 9}      # fewest owned last edges of a perfect assignment
MIXED, NONE, ONE, BOTH = 0, 1, 2, 3
ORDERED = 1 << 30


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("regular_waves")
    exes = {}
    for name in ("regular_waves_main", "regular_place_main"):
        exes[name] = str(d / name)
        subprocess.run([RP.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", RP.CSRC, os.path.join(HERE, name + ".cpp"), "-o", exes[name]], check=True)

    def run(name, graphs, force_s=0):
        return subprocess.run([exes[name], str(force_s), "0"], input=RP.text_of(graphs), capture_output=True, text=True, check=True).stdout
    return run


def parse(out, graphs):
    lines, res, at = out.splitlines(), [], 0

    def cost(ln, tag):
        w = ln.split()
        assert w[0] == tag and len(w) == 1 + 5 + 14
        return dict(zip(RP.COST_KEYS, map(int, w[1:6])), streams=[int(x) for x in w[6:]])

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
        r = dict(zip(("S", "TS", "block", "placed"), map(int, head[1:])))
        for tag, key in (("minlast", "minlast"), ("waves", "waves"), ("thread_of", "thread_of")):
            w = lines[at + 1].split()
            assert w[0] == tag
            r[key] = [int(x) for x in w[1:]]
            at += 1
        at += 1
        if r["placed"]:
            r["identity"], r["ordered"] = cost(lines[at], "identity"), cost(lines[at + 1], "ordered")
            at += 2
        r["old"], r["own"] = table(m, 16), table(m, 16)
        r["rec"] = table(r["block"], WORDS) if r["placed"] else None
        res.append(r)
    assert at == len(lines)
    return res


@pytest.fixture(scope="module")
def tables(programs):
    G = RP.all_graphs()
    out = {}
    for fs in FORCED_S:
        for (name, g), r in zip(G.items(), parse(programs("regular_waves_main", list(G.values()), fs), list(G.values()))):
            out[name, fs] = (g, r)
    return out


def some(tables):
    return {k: v for k, v in tables.items() if v[1] is not None}


def classes_of(own):
    last = own[:, 14]
    return np.where(last == 0, NONE, np.where(last == 3, BOTH, ONE))


def test_the_assignment_is_perfect_and_in_canonical_order(tables):
    for (name, fs), ((m, n, ip, ix), r) in some(tables).items():
        own = r["own"]
        assert sorted(own[:, 0:2].ravel().tolist()) == list(range(n)), name
        rows = RP.rows_of_columns(m, n, ip, ix)
        for i in range(m):
            csr = set(int(c) for c in ix[ip[i]:ip[i + 1]])
            assert int(own[i, 0]) in csr and int(own[i, 1]) in csr and own[i, 0] != own[i, 1], (name, i)
            last = [rows[int(own[i, v])][-1] == i for v in range(2)]
            assert int(own[i, 14]) == last[0] + 2 * last[1], (name, i)
            assert last != [True, False], (name, i)                                   # exactly one last edge: it is column 1
        assert set(own[:, 14].tolist()) <= {0, 2, 3}, name
        count = [int((classes_of(own) == c).sum()) for c in (NONE, ONE, BOTH)]
        assert r["minlast"] == [count[1] + 2 * count[2]] + count, name


def test_it_owns_as_few_last_edges_as_a_min_cost_solve(tables):
    from scipy.optimize import linear_sum_assignment
    seen = set()
    for (name, fs), ((m, n, ip, ix), r) in some(tables).items():
        if name in seen:
            continue
        seen.add(name)
        # columns against two places per check: 0 for a check of the column, 1 where it is the column's highest, a wall elsewhere
        rows = RP.rows_of_columns(m, n, ip, ix)
        cost = np.full((n, 2 * m), 10 ** 6, np.int64)
        for j in range(n):
            for i in rows[j]:
                cost[j, 2 * i:2 * i + 2] = 1 if i == rows[j][-1] else 0
        a, b = linear_sum_assignment(cost)
        best = int(cost[a, b].sum())
        assert best < 10 ** 6 and r["minlast"][0] == best, (name, r["minlast"], best)
        if name in MIN_LAST:
            assert best == MIN_LAST[name], name
    assert set(MIN_LAST) <= seen


def test_the_thread_map_is_a_bijection_and_the_labels_hold(tables):
    for (name, fs), ((m, *_), r) in some(tables).items():
        S, block, cls = r["S"], r["block"], classes_of(r["own"])
        t = np.array(r["thread_of"])
        assert len(t) == S * m and len(set(t.tolist())) == S * m and t.min() >= 0 and t.max() < block, (name, fs)
        assert len(r["waves"]) == block // 64, (name, fs)
        held = [set() for _ in range(block // 64)]
        for item, thread in enumerate(t.tolist()):
            held[thread // 64].add(int(cls[item % m]))
        for w, label in enumerate(r["waves"]):
            if label != MIXED:
                assert held[w] <= {label}, (name, fs, w)
            else:
                assert len(held[w]) != 1, (name, fs, w)                               # a wave of one class is labelled by it
    (g, r) = tables["bb144_Hx", 0]
    assert r["S"] == 7 and len(r["waves"]) == 8 and sum(w != MIXED for w in r["waves"]) >= 6


def test_the_ordered_table_is_wired_as_the_graph_says(tables):
    seen = 0
    for (name, fs), ((m, n, ip, ix), r) in some(tables).items():
        if not r["placed"]:
            continue
        S, block, rec, own = r["S"], r["block"], r["rec"], r["own"]
        t = np.array(r["thread_of"])
        spare = sorted(set(range(block)) - set(t.tolist()))
        w15 = rec[:, 15]
        assert ((w15 & ORDERED) != 0).all(), name
        assert ((w15 >> 24) & 3).tolist() == [r["waves"][x // 64] for x in range(block)], name
        slot, member = (w15 >> 12) & 0xfff, w15 & 0xfff
        for s in range(S):
            assert (slot[t[s * m:(s + 1) * m]] == s).all() and (member[t[s * m:(s + 1) * m]] == np.arange(m)).all(), (name, s)
        assert (slot[spare] == S).all(), name
        # the wiring test of the placement, on the records put back into the identity order (team lanes slot-major, then the lanes of no team)
        back = np.concatenate([rec[t], rec[spare]]) if spare else rec[t]
        back = back.copy()
        back[:, 15] = 0
        RP.assert_table_is_consistent((name, fs), (m, n, ip, ix), dict(r, span=S * m * (RST + 2) * 8, offD=0), back, linear=False)
        seen += 1
    assert seen >= 20


def test_the_gathers_and_message_stores_stay_conflict_free(tables):
    for (name, fs), (g, r) in some(tables).items():
        if not r["placed"]:
            continue
        block, c = r["block"], r["ordered"]
        cyc, over = RP.model(r["rec"], block)                                         # lane groups are consecutive threads: the record's own order
        assert cyc == c["streams"], name
        assert cyc[0:8] == [block // 32] * 8 and c["gather"] == 8 * (block // 32), name
        assert sum(cyc[10:14]) == 4 * (block // 16) and sum(over[10:14]) == 0 and c["msg_over6"] == 0, name
        assert c["post_over6"] == sum(over[8:10]), name


def test_the_posterior_stores_are_no_worse_than_in_the_identity_order(tables):
    """Cycles above 6 per posterior-store instruction, per workgroup pass: the ordered table against the bank-model assignment's table in the identity
    order, per graph and shape.  One Kempe walk under the order left 1 or 2 cycles on bb72, bb288, bb90 and r63_m36 where the identity order has none;
    thread swaps inside a 32-lane group and up to four walks (csrc/regular_place.h) end at 0 on every BB matrix (identity -> ordered: bb72 0 -> 0,
    bb144 1 -> 0, bb288 0 -> 0, bb90 0 -> 0, bb108 1 -> 0, r63_m36 0 -> 0, r63_m512 29 -> 25)."""
    worse = []
    for (name, fs), (g, r) in some(tables).items():
        if not r["placed"]:
            continue
        c = r["ordered"]
        print(f"{name} S {r['S']} block {r['block']}: posterior stores {r['identity']['post_store']} -> {c['post_store']}, above 6 per instruction "
              f"{r['identity']['post_over6']} -> {c['post_over6']}")
        if c["post_over6"] > r["identity"]["post_over6"]:
            worse.append((name, fs, r["identity"]["post_over6"], c["post_over6"]))
    assert not worse, worse


def test_the_bank_model_assignment_is_unchanged(programs, tables):
    """tests/golden/regular_own_words.json: SHA-256 of the little-endian int32 words of the bank-model ownership table and of its placement in the identity
    order at the plan's own S, per graph, recorded before the min-last assignment existed"""
    import hashlib
    import json
    with open(os.path.join(HERE, "golden", "regular_own_words.json")) as fh:
        gold = json.load(fh)
    G = RP.all_graphs()
    assert set(gold) == set(G)
    old = RP.parse(programs("regular_place_main", list(G.values()), 0), list(G.values()))
    for (name, g), r in zip(G.items(), old):
        if r is None:
            assert tables[name, 0][1] is None and gold[name] is None, name
            continue
        assert np.array_equal(r["own"], tables[name, 0][1]["old"]), name
        assert hashlib.sha256(r["own"].astype("<i4").tobytes()).hexdigest() == gold[name]["own_sha256"], name
        if r["placed"]:
            assert (r["rec"][:, 15] == 0).all(), name                                  # the identity order: no (slot, member) word, every wave mixed
            assert hashlib.sha256(r["rec"].astype("<i4").tobytes()).hexdigest() == gold[name]["placed_sha256"], name
            assert r["cost"]["post_over6"] == gold[name]["post_over6"], name
