"""The elimination cases of tests/elim_shapes.py hold what they are named for (no GPU): the oracle's two routines agree with a plain numpy elimination on the
reduced matrix, the right-hand side and the pivots of every shot, and rank, number of row swaps and the last pivot's column are the ones the table states."""
import numpy as np
import pytest

import elim_shapes as E


@pytest.mark.parametrize("name", list(E.TABLE))
def test_case_holds_what_it_is_named_for(oracle, name):
    c = E.case(name)
    assert c.lds == 5 * c.m + 8 * c.nwords + 40 and c.refused == (c.lds > E.ELIM_MAX)
    for s in range(c.B):
        A, b, pr, pc, swaps = E.plain_elimination(c.A[s], c.b[s])
        oA, ob, opr, opc = oracle.gf2_elimination(c.A[s], c.b[s])
        assert np.array_equal(A, oA) and np.array_equal(b, ob) and list(opr) == pr and list(opc) == pc, (name, s)
        pP, pb, ppr, ppc = oracle.gf2_elimination_packed(c.A[s], c.b[s])
        assert np.array_equal(pP, oracle.pack_rows_u64(A)) and np.array_equal(pb, b) and list(ppr) == pr and list(ppc) == pc, (name, s)
        if not c.refused:
            assert (len(pr), swaps, pc[-1] if pc else -1) == (c.expect["rank"][s], c.expect["swaps"][s], c.expect["last"][s]), (name, s)
        assert pr == list(range(len(pr)))


def test_the_table_covers_the_edges():
    T = {n: E.case(n) for n in E.TABLE}
    assert (E.block_of(T["e511x40"].m), E.block_of(T["e512x40"].m)) == (256, 1024) and T["e512x40"].m - T["e511x40"].m == 1
    assert [T[n].lds for n in ("lds_13097", "lds_13098", "lds_30710", "lds_30711")] == [65533, 65538, 153598, 153603]
    assert T["lds_13097"].lds <= 64 * 1024 < T["lds_13098"].lds and T["lds_30710"].lds <= E.ELIM_MAX < T["lds_30711"].lds
    assert [n for n in T if T[n].refused] == ["lds_30711"] and all(T[n].n == 8 for n in T if n.startswith("lds_"))
    assert {(T[n].m, T[n].n) for n in ("e1x1", "e1x64", "e64x1")} == {(1, 1), (1, 64), (64, 1)}
    a = T["antidiag65"].A[0]
    assert a.shape == (65, 65) and np.array_equal(a, a.T) and a.sum() == 65 and all(a[i, 64 - i] for i in range(65))
    z = T["zero_first"]
    assert not z.A[0, 0].any() and z.expect["rank"] == [z.n] == [z.m - 1] and z.expect["swaps"] == [z.n]     # the empty row is handed down at every pivot
    for name, n in (("last_col64", 64), ("last_col65", 65)):
        c = T[name]
        assert c.n == n and c.expect["last"] == [n - 1] and c.A[0, 2].sum() == 1 and c.A[0, 2, n - 1] == 1
    assert T["ones70"].A.all() and T["ones70"].nwords == 2
    b5 = T["batch5"]
    assert b5.B == 5 and b5.expect["rank"][:3] == [min(b5.m, b5.n), 0, 1] and all(1 < r < min(b5.m, b5.n) for r in b5.expect["rank"][3:]) and not b5.A[1].any()
    assert T["shift65"].expect["swaps"] == [64]


def test_packed3_has_bits_beyond_n_that_never_pivot(oracle):
    P, b, n = E.packed3()
    assert P.shape == (1, 30, 3) and n == 70 and E.nwords_of(n) == 2
    beyond = (P[0, :, 1] >> np.uint64(6)).astype(bool) | P[0, :, 2].astype(bool)
    assert beyond.all()
    oP, ob, pr, pc = oracle.gf2_elimination_packed_words(P[0], b[0], n)
    assert len(pr) == 29 and pc.max() < n and (pc[-1], list(pr)) == (31, list(range(29)))        # row 4 = row 1 + row 2
    assert not oP[29].any() and oP[:29, 2].astype(bool).any()                                # the third word is carried along and cleared with its row
    # the same matrix cut to its 70 columns gives the same pivots and right-hand side: the bits beyond n changed nothing that is reported
    cols = np.array([[(int(P[0, r, c >> 6]) >> (c & 63)) & 1 for c in range(n)] for r in range(30)], np.uint8)
    _, cb, cpr, cpc = oracle.gf2_elimination_packed(cols, b[0])
    assert np.array_equal(cb, ob) and np.array_equal(cpr, pr) and np.array_equal(cpc, pc)
