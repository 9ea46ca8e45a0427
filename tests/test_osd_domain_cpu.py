"""The OSD-0 cases of tests/osd_shapes.py have the properties they are named for (no GPU; the oracle and plain numpy only): every family has the rank
and the dependency its label says, every shot lies on the side of the column space its class says, the oracle equals a literal numpy restatement of
the reference on the small families, and the mirror of the dispatch (rule_path) gives hand-computed answers on both sides of every boundary."""
import numpy as np
import pytest

import osd_shapes as OS

NAMES = list(OS.TABLE)
RUN = [n for n in NAMES if n != "refused"]


def test_the_table_is_what_the_mirror_says():
    """every label equals rule_path on the family's own (m, n, max_col_deg); every flag family has a flag that changes something"""
    for name in NAMES:
        f = OS.family(name)
        r = OS.rule_path(f.m, f.n, f.max_col_deg)
        assert (r.path, r.w16, r.refused) == (f.path, f.w16, f.refused), name
        if f.kind == "heavy":
            assert f.max_col_deg == OS.TABLE[name][3], name
        elif f.kind != "empty" and name != "tiny130x9":
            assert f.max_col_deg == (3 if name == "m4096" else 4), name          # (the edges N_GJ_* are computed for weight 4)
    for name in OS.FLAG_FAMILIES:
        assert OS.honoured(OS.family(name)), name
    for name in OS.PRESORT_FAMILIES:
        assert OS.family(name).path in ("GJ", "GJG")
    assert not set(OS.GROUPS["wide"]) & set(OS.GROUPS["tall"])
    assert all(OS.family(n).n >= 65534 for n in OS.GROUPS["wide"]) and all(OS.family(n).m >= 4095 for n in OS.GROUPS["tall"])
    assert [n for n in NAMES if OS.family(n).n >= 65534] == list(OS.GROUPS["wide"])


def numpy_rank(A):
    A = A.copy()
    m, n = A.shape
    row = 0
    for col in range(n):
        nz = np.flatnonzero(A[row:, col])
        if nz.size == 0:
            continue
        p = row + nz[0]
        A[[row, p]] = A[[p, row]]
        rest = row + 1 + np.flatnonzero(A[row + 1:, col])
        A[rest] ^= A[row]
        row += 1
        if row == m:
            break
    return row


@pytest.mark.parametrize("name", NAMES)
def test_family_rank_and_dependency(oracle, name):
    f = OS.family(name)
    A = OS.dense(f)
    assert A.shape == (f.m, f.n) and int(A.sum()) == f.indices.size
    _, _, prow, _ = oracle.gf2_elimination_packed(A, np.zeros(f.m, np.uint8))
    assert len(prow) == f.rank, (name, len(prow))
    if f.m <= 300:
        assert numpy_rank(A) == f.rank, name
    if f.null_rows is not None:
        assert not np.bitwise_xor.reduce(A[list(f.null_rows)], axis=0).any(), name       # the witness: these rows sum to zero
        assert f.rank < f.m
    if name.startswith("ident"):
        assert f.rank == f.m
    if name == "tall300x40":
        assert f.rank == f.n
    if name == "halfdup256":
        assert np.array_equal(A[:128], A[128:])
    if name == "doubled200":
        assert np.array_equal(A[:, 0::2], A[:, 1::2])


@pytest.mark.parametrize("name", RUN)
def test_every_shot_is_on_its_side_of_the_column_space(oracle, name):
    """classes other than the random syndrome: the oracle's solution reproduces the syndrome (all of them are in the column space; the issue's
    classes 1-3 among them); random syndrome: it does not.  Every shot, no leave-outs."""
    f = OS.family(name)
    want = OS.solutions(oracle, name)
    assert ("random syndrome" in OS.shots(name)) == (f.rank < f.m and f.null_rows is not None)
    for (cls, synd, llr, hard, ordering), w in zip(OS.batches(name), want):
        assert len(cls) == synd.shape[0] == w.shape[0] and set(np.unique(w)) <= {0, 1}
        back = OS._syndromes(f, w)
        ok = (back == synd).all(axis=1)
        rs = cls == "random syndrome"
        assert ok[~rs].all(), (name, [(int(b), cls[b]) for b in np.flatnonzero(~ok & ~rs)])
        assert not ok[rs].any(), (name, np.flatnonzero(ok & rs))
        if rs.any():
            assert OS.outside(f, synd[rs]).all()
    S = OS.shots(name)
    h = S["hard solves"]
    assert np.array_equal(OS._syndromes(f, h.hard), h.synd)                # the sweep has nothing to do
    z = S["all zero"]
    assert not z.synd.any() and not z.hard.any() and not z.llr.any()
    nf = S["non-finite llr"].llr
    if f.n >= 6:
        assert np.isnan(nf).any(axis=1).all() and np.isposinf(nf).any(axis=1).all() and np.isneginf(nf).any(axis=1).all()
        assert ((nf == 0) & np.signbit(nf)).any(axis=1).all() and ((nf != 0) & (np.abs(nf) < 2.3e-308)).any(axis=1).all()
    assert np.array_equal(np.sort(S["explicit ordering"].ordering, axis=1), np.broadcast_to(np.arange(f.n), (OS.SHOTS, f.n)))


def restated_osd0(H, syndrome, llr, hard, ordering=None):
    """osd.py:5-29 in plain numpy: residual syndrome, stable argsort of |llr| (NaN as +inf: the rule of qldpc_osd0_batch), the column-by-column
    elimination of kernels.py:48-96 with the first row at or below the diagonal as the pivot, back-fill."""
    m, n = H.shape
    s = (syndrome + H.astype(np.int64) @ hard) % 2
    if ordering is None:
        a = np.abs(llr)
        ordering = np.argsort(np.where(np.isnan(a), np.inf, a), kind="stable")
    A = np.ascontiguousarray(H[:, ordering])
    s = s.astype(np.uint8)
    row, prow, pcol = 0, [], []
    for col in range(n):
        if row >= m:
            break
        nz = np.flatnonzero(A[row:, col])
        if nz.size == 0:
            continue
        p = row + nz[0]
        if p != row:
            A[[row, p]] = A[[p, row]]
            s[[row, p]] = s[[p, row]]
        rest = np.flatnonzero(A[:, col])
        rest = rest[rest != row]
        A[rest, col:] ^= A[row, col:]
        s[rest] ^= s[row]
        prow.append(row)
        pcol.append(col)
        row += 1
    e = np.zeros(n, np.int64)
    e[ordering[pcol]] = s[prow]
    return ((hard + e) % 2).astype(np.int8)


@pytest.mark.parametrize("name", [n for n in RUN if OS.TABLE[n][1] <= 300])
def test_oracle_equals_the_restated_reference_on_small_families(oracle, name):
    """every shot where n <= 2048; beyond (the python loop walks every column) the first shot of every class"""
    f = OS.family(name)
    H = OS.dense(f)
    for (cls, synd, llr, hard, ordering), w in zip(OS.batches(name), OS.solutions(oracle, name)):
        pick = range(len(cls)) if f.n <= 2048 else range(0, len(cls), OS.SHOTS)
        for b in pick:
            got = restated_osd0(H, synd[b], llr[b], hard[b], None if ordering is None else ordering[b])
            assert np.array_equal(got, w[b]), (name, b, cls[b])


def test_rule_path_at_hand_computed_points():
    """Both sides of every boundary of the dispatch, worked out on paper from the formulas of csrc/osd_plan.h (the byte totals are in the comments)."""
    R, LDS, UG, RE, GL = OS.rule_path, OS.FLAG_OSD_LDS, OS.FLAG_OSD_UG, OS.FLAG_OSD_REFORDER, OS.FLAG_OSD_GLOBAL

    def what(m, n, cd, flags=0):
        r = R(m, n, cd, flags)
        return r.path, r.w16, r.block, r.mode, r.redo
    # the one-wave kernel: m <= 128 && n <= 1024, unless a size-class flag asks for another kernel (REFORDER does not)
    assert what(128, 1024, 4) == ("SMALL", False, 64, 0, False)
    assert what(129, 1024, 4) == ("GJ", False, 256, 1, True)
    assert what(128, 1025, 4) == ("GJ", False, 256, 1, True)
    assert what(128, 1024, 4, LDS) == ("GJ", False, 256, 1, True)
    assert what(128, 1024, 4, RE) == ("SMALL", False, 64, 0, False)
    assert what(128, 1024, 4, RE | LDS) == ("REFORDER_LDS", False, 256, 1, False)
    assert what(129, 1024, 4, RE) == ("REFORDER_LDS", False, 256, 1, False)
    # threads: round_up(max(m + 2, 256), 64) capped at 1024; W16 = 16 row words at 1024 threads
    assert [what(m, 2400, 4)[1:3] for m in (254, 255, 958, 959, 960, 961)] == [(False, 256), (False, 320), (False, 960), (False, 1024), (False, 1024), (True, 1024)]
    assert [what(m, 2560, 4)[:3] for m in (1022, 1023, 1024, 1025)] == [("GJ", True, 1024)] * 3 + [("GJG", False, 1024)]
    assert what(1024, 2560, 4, UG) == ("GJG", False, 1024, 2, True)
    assert what(1024, 2560, 4, UG | RE) == ("REFORDER_UG", False, 1024, 2, False)
    assert what(1025, 2200, 4, RE) == ("REFORDER_UG", False, 1024, 2, False)
    # m <= 4096 for everything with a row transform
    assert what(4096, 5000, 4) == ("GJG", False, 1024, 2, True)
    assert what(4097, 5000, 4) == ("GLOBAL", False, 1024, 0, False)
    assert what(4097, 5000, 4, UG | RE) == ("GLOBAL", False, 1024, 0, False)
    assert what(4096, 5000, 4, GL) == ("GLOBAL", False, 1024, 0, False)
    assert what(300, 700, 4, GL) == ("GLOBAL", False, 256, 0, False)
    # osd_gj by n at m = 200, weight 4: round_up(12 n + 16528, 16) + 15056 <= 163840  <=>  n <= 11021
    assert OS.gj_lds(200, 11021, 4) == 163840 and OS.gj_lds(200, 11022, 4) == 163856
    assert OS.N_GJ_200 == 11021 and what(200, 11021, 4)[0] == "GJ" and what(200, 11022, 4) == ("GJG", False, 1024, 1, True)
    # at m = 1008 (16 words): round_up(12 n + 16528, 16) + 26128 <= 163840  <=>  n <= 10098 (137704 -> 137712; one more column: 137716 -> 137728)
    assert OS.gj_lds(1008, 10098, 4) == 163840 and OS.gj_lds(1008, 10099, 4) == 163856
    assert OS.N_GJ_1008 == 10098 and what(1008, 10098, 4)[:2] == ("GJ", True) and what(1008, 10099, 4)[:2] == ("GJG", False)
    # the uint16 tables: n < 65535
    assert what(200, 65534, 4) == ("GJG", False, 1024, 2, True)
    assert what(200, 65535, 4) == ("GLOBAL", False, 1024, 0, False) and what(129, 65535, 4)[0] == "GLOBAL"
    # a heavy column at m = 300, n = 700: osd_gj 32976 + 2048 d, osd_gjg 22624 + 2048 d, the reference-order kernel's mode 2 21320 + 2048 d
    assert (OS.gj_lds(300, 700, 63), OS.gj_lds(300, 700, 64)) == (162000, 164048)
    assert (OS.gjg_lds(300, 700, 68), OS.gjg_lds(300, 700, 69)) == (161888, 163936)
    assert (OS.reforder_lds(300, 700, 69, 2), OS.reforder_lds(300, 700, 70, 2)) == (162632, 164680)
    assert (OS.D_GJ_300, OS.D_GJG_300, OS.D_UG_300) == (63, 68, 69)
    assert [what(300, 700, d)[0] for d in (63, 64, 68, 69, 70)] == ["GJ", "GJG", "GJG", "REFORDER_UG", "GLOBAL"]
    assert what(300, 700, 69) == ("REFORDER_UG", False, 1024, 2, False)
    # and at m = 1008, n = 2500: osd_gj 147216 + 2048 d
    assert (OS.gj_lds(1008, 2500, 8), OS.gj_lds(1008, 2500, 9)) == (163600, 165648) and OS.D_GJ_1008 == 8
    assert what(1008, 2500, 8)[:2] == ("GJ", True) and what(1008, 2500, 9) == ("GJG", False, 1024, 1, True)
    # the global kernel's own limit: 5 m + 8 nwords + 40 <= 153600, one row word for n = 64  <=>  m <= 30710
    assert OS.elim_lds(30710, 64) == 153598 and OS.elim_lds(30711, 64) == 153603 and OS.elim_lds(30720, 64) == 153648
    assert not R(30710, 64, 4).refused and R(30710, 64, 4).path == "GLOBAL" and R(30711, 64, 4).refused
    assert R(30720, 64, 4).refused and R(30720, 64, 4).path == "NONE"
    # nothing to do
    assert R(0, 5, 0).path == "NONE" and R(5, 0, 0).path == "NONE" and not R(0, 5, 0).refused


def test_mirror_reproduces_the_three_budgets_at_circ144():
    """the production Z sector, 1008 x 8785 with columns of weight <= 6: the totals worked out by hand from the three layouts of csrc/osd_plan.h"""
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ144")
    m, n = len(d["HdecZ_indptr"]) - 1, int(d["HdecZ_shape"][1])
    cd = int(np.bincount(d["HdecZ_indices"], minlength=n).max())
    assert (m, n, cd) == (1008, 8785, 6)
    # osd_gj: U 1010 * 16 * 8 = 129280 (> sort 121948) + 3072 + 12288 + 4032 + 6144 + 256 + 368 + 4048 + 16
    assert OS.gj_lds(m, n, cd) == 159504
    # osd_gjg: 16512 + 3072 + 12288 + 4032 + 2048 + 1024 + 160 + 16
    assert OS.gjg_lds(m, n, cd) == 39152
    # osd_ref_layout: mode 1 129280 + 3072 + 12288 + 2016 + 2048 + 416 + 64 + 16; mode 2 the same without U plus 16512
    assert (OS.reforder_lds(m, n, cd, 1), OS.reforder_lds(m, n, cd, 2)) == (149200, 36432)
    r = OS.rule_path(m, n, cd)
    assert (r.path, r.w16, r.block, r.mode, r.redo) == ("GJ", True, 1024, 1, True)


def test_path_constants_follow_the_header():
    """Every QLDPC_OSD_PATH_* / QLDPC_OSD_DETAIL_* of include/qldpc_hip.h has a `_lib.OSD_*` twin with the same value, and the other way round."""
    import re
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    paths = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+QLDPC_OSD_PATH_(\w+)\s+(\(?-?\d+\)?)", text)}
    bits = {k: int(v, 16) for k, v in re.findall(r"#define\s+QLDPC_OSD_DETAIL_(\w+)\s+(0x[0-9a-fA-F]+)", text)}
    assert set(paths) == {"NONE", "SMALL", "GJ", "GJG", "REFORDER_LDS", "REFORDER_UG", "GLOBAL"} and sorted(paths.values()) == list(range(-1, 6))
    assert bits == {"MODE_MASK": 0x3, "REDO": 0x4}
    for name, v in paths.items():
        assert getattr(_lib, "OSD_PATH_" + name) == v, name
    for name, v in bits.items():
        assert getattr(_lib, "OSD_DETAIL_" + name) == v, name
    assert {k[9:] for k in vars(_lib) if k.startswith("OSD_PATH_")} == set(paths)
    assert {k[11:] for k in vars(_lib) if k.startswith("OSD_DETAIL_")} == set(bits)
    assert "qldpc_osd0_last_path" in _lib.exports()
