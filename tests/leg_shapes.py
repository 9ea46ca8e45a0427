"""Graph shapes for BP with guided decimation (csrc/decimation.hip) and the leg and launch it shares with Relay-BP (csrc/bp_leg.h, csrc/relay_bp.hip).

cases() is every family of tests/graph_shapes.py that the two decoders accept (row degree <= 56) plus families of its own, each of which sits on one
line that belongs to these two kernels alone: the four LDS limits (BPGD's count and Relay-BP's count, each with the posteriors in LDS and in global
memory), the plane-word boundaries of the two bit planes below one wave (n = 1, 31, 32, 33), and a tie class that spans every wave of the selection
with eight and with sixteen waves.  tests/test_leg_shapes_cpu.py checks the structure, the place of every family relative to its limit and that the
numpy model's runs contain the edges the GPU module is about; tests/test_leg_shapes_gpu.py pins both kernels to their models on every case.  Plain
module (no pytest hooks); deterministic from the seed; CSR rows sorted, no repeated edges.

The byte counts and the block rule below are a SECOND COPY of the host code (leg_lds_prefix and shot_queue_launch of bp_leg.h, relay_lds_bytes and
relay_mode of relay_bp.hip, decim_lds_bytes and decim_mode of decimation.hip), kept on purpose as an independent statement of the rules.  Every new
family is sized by searching these functions, never by a literal, and the GPU module observes the accept / refuse lines directly, so a limit that
moves in csrc/ fails there and has to be moved here too.
"""
import zlib
from types import SimpleNamespace

import numpy as np

import decimation_model as DM
import graph_shapes as GS

LDS_BYTES = 160 * 1024
LEG_ROW_DEG = 56                                  # bits 0-55 of the packed check record hold the input signs
BLOCK_SMALL, BLOCK_LARGE, BLOCK_M, BLOCK_N = 512, 1024, 512, 4096
SELECT_BYTES = 2 * 16 * 8 + 2 * 16 * 4            # BPGD: two alternating buffers of sixteen per-wave candidates (64-bit key, 32-bit column)

# (alpha, clip_llr, t_round, max_rounds, per_round, fix_llr)
DECIM_SETS = {
    "3x4x64": dict(alpha=0.875, clip_llr=20.0, t_round=3, max_rounds=4, per_round=64, fix_llr=25.0),
    # fix_llr below clip_llr and below some priors: the messages can outweigh a frozen prior, so a frozen decision can flip
    "1x40x1": dict(alpha=1.0, clip_llr=20.0, t_round=1, max_rounds=40, per_round=1, fix_llr=5.0),
    "6x3x7": dict(alpha=0.625, clip_llr=6.5, t_round=6, max_rounds=3, per_round=7, fix_llr=1000.0),
}
RELAY_SCALED = dict(t0=20, tr=10, max_legs=20)    # PARAM_SETS["scaled"] of tests/test_relay_gpu.py (the GPU module asserts that they are equal)
RELAY_CALL = (20261016, 3, 1)                     # seed, shot_begin, tag
B = 4
TIE_PRIOR = 100.0


def _up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------- the rules, restated
def leg_lds_prefix(m, n, vg):
    """V[n] f64 (not in the global-memory form) | 16 bytes per check (alpha * min1, alpha * min2) | 8 bytes per check (signs, argmin)."""
    off_p = 0 if vg else _up(8 * n, 16)
    off_i = off_p + 16 * m
    return _up(off_i + 8 * m, 16)


def relay_lds_bytes(m, n, vg):
    """the prefix | one 16-bit draw per column, padded to four columns | 32 bytes of flags"""
    return _up(leg_lds_prefix(m, n, vg) + _up(n, 4) * 2, 16) + 32


def decim_lds_bytes(m, n, vg):
    """the prefix | two bit planes of ceil(n / 32) words, each padded to 16 bytes | 16 bytes of flags | the per-wave candidates"""
    plane = _up((n + 31) // 32 * 4, 16)
    return leg_lds_prefix(m, n, vg) + 2 * plane + 16 + SELECT_BYTES


def _tables(n, max_row_deg):
    return n < 65535 and max_row_deg < 256            # graph.hip: the slot tables exist


def relay_mode(m, n, max_row_deg):
    """0: refused, 1: everything in LDS, 2: posteriors in global memory."""
    if not _tables(n, max_row_deg) or m <= 0 or n <= 0 or max_row_deg > LEG_ROW_DEG:
        return 0
    if relay_lds_bytes(m, n, False) <= LDS_BYTES:
        return 1
    return 2 if relay_lds_bytes(m, n, True) <= LDS_BYTES else 0


def decim_mode(m, n, max_row_deg):
    """As relay_mode with BPGD's own count; a graph Relay-BP refuses is refused here too."""
    if relay_mode(m, n, max_row_deg) == 0:
        return 0
    if decim_lds_bytes(m, n, False) <= LDS_BYTES:
        return 1
    return 2 if decim_lds_bytes(m, n, True) <= LDS_BYTES else 0


def block_threads(m, n):
    """shot_queue_launch: 512 threads up to (m, n) = (512, 4096), 1024 beyond either."""
    return BLOCK_LARGE if m > BLOCK_M or n > BLOCK_N else BLOCK_SMALL


def modes(c):
    """(BPGD, Relay-BP)"""
    rd = int(c.row_deg.max()) if c.m else 0
    return decim_mode(c.m, c.n, rd), relay_mode(c.m, c.n, rd)


def _last(ok, lo, hi):
    """the last x in lo .. hi with ok(x), which is followed by one without"""
    x = max(v for v in range(lo, hi) if ok(v))
    assert x + 1 < hi and not ok(x + 1)
    return x


# ---------------------------------------------------------------------------------------- the cases
WIDE_PRIORS = ("above clip", "zero class", "negative class", "one -0.0")      # of alldeg_wide's seven (n = 5000, the slowest model runs)


def _case(name, ip, ix, n, priors, claims, err_weight=3, relay=True, new=True, pinned_syndrome=None):
    rd, cd = GS.degrees(ip, ix, n)
    return SimpleNamespace(name=name, seed=zlib.crc32(name.encode()), indptr=ip, indices=ix, n=int(n), m=len(ip) - 1, nnz=len(ix), priors=priors,
                           row_deg=rd, col_deg=cd, claims=claims, err_weight=err_weight, pinned_syndrome=pinned_syndrome or {}, new=new,
                           relay_here=relay)


def cases(seed=20261019):
    """-> list of cases (SimpleNamespace): name, seed, indptr, indices, n, m, nnz, priors {name: finite array}, row_deg, col_deg, claims (structure and
    modes the CPU suite verifies), err_weight, pinned_syndrome (both read by graph_shapes.syndromes), new (a family of this module), relay_here (the
    GPU module decodes it with Relay-BP: tests/test_wg_shapes_gpu.py does not)."""
    out = []
    for c in GS.families():
        if c.row_deg.max() > LEG_ROW_DEG:
            continue
        priors = {k: v for k, v in c.priors.items() if np.isfinite(v).all() and (c.name != "alldeg_wide" or k in WIDE_PRIORS)}
        out.append(_case(c.name, c.indptr, c.indices, c.n, priors, {}, err_weight=c.err_weight, relay=not c.relay, new=False,
                         pinned_syndrome=c.pinned_syndrome))

    def rng_of(name):
        return np.random.default_rng([seed, zlib.crc32(name.encode())])

    def normal(n):
        return rng_of("normal").normal(2.5, 1.0, n)

    # ---- posteriors in LDS or in global memory (modes 1 / 2), by BPGD's count and by Relay-BP's: m = 300 as the vglobal_* families, 3000 columns
    # with edges among n, a first row of degree 56; the two graphs of a pair differ in one degree-0 column
    m = 300
    for who, count in (("decim", decim_lds_bytes), ("relay", relay_lds_bytes)):
        n_last = _last(lambda n: count(m, n, False) <= LDS_BYTES, 12000, 24000)
        cd = np.append(GS.blocks(rng_of(who + "_lds"), (4, 1500), (2, 1500), (0, n_last - 3000)), 0)      # the extra column has degree 0
        for tag, n in (("last", n_last), ("first", n_last + 1)):
            ip, ix = GS.deal(rng_of(who + "_lds/graph"), m, cd[:n], fixed={0: np.flatnonzero(cd > 0)[:56]})
            name = f"{who}_lds_{tag}"
            out.append(_case(name, ip, ix, n, {"normal": normal(n), "uniform": np.full(n, 4.0)},
                             dict(m=m, n=n, max_row=56, deg0=n - 3000, line=dict(count=who, limit="lds", fits=(tag == "last")),
                                  modes={"decim_lds_last": (1, 2), "decim_lds_first": (2, 2), "relay_lds_last": (1, 1), "relay_lds_first": (1, 2)}[name]),
                             err_weight=8))
    # ---- accepted or refused (modes 2 / 0) at n = 64: about 200 rows of degree 5 scattered over the m rows, every other row empty; column degree
    # about 16, m far above the 1024 threads.  The two graphs of a pair differ in one empty last row.
    n = 64
    for who, count in (("decim", decim_lds_bytes), ("relay", relay_lds_bytes)):
        m_last = _last(lambda m: count(m, n, True) <= LDS_BYTES, 4000, 9000)
        full = np.sort(rng_of(who + "_vg").choice(m_last, 200, replace=False))
        for tag, m in (("vg_last", m_last), ("refused", m_last + 1)):
            empty = {i: [] for i in np.setdiff1d(np.arange(m), full).tolist()}
            r = rng_of(who + "_vg/cd")
            cd = np.full(n, 15)
            cd[r.choice(n, 40, replace=False)] = 16                        # 24 * 15 + 40 * 16 = 1000 stubs for 200 rows of 5
            ip, ix = GS.deal(rng_of(who + "_vg/graph"), m, cd, fixed=empty, row_cap=5)
            name = f"{who}_{tag}"
            out.append(_case(name, ip, ix, n, {"three values": GS.by_class(rng_of("vg3"), n, [-1.5, 1.7, 4.0], sizes=[8, 16, 40])},
                             dict(m=m, n=n, full_rows=200, full_deg=5, line=dict(count=who, limit="vg", fits=(tag == "vg_last")),
                                  modes={"decim_vg_last": (2, 2), "decim_refused": (0, 2), "relay_vg_last": (0, 2), "relay_refused": (0, 0)}[name]),
                             err_weight=2))
    # ---- the plane-word boundaries below one wave: one word not full, exactly one, one bit of a second; n = 1 is a single degree-1 check
    out.append(_case("n1", np.array([0, 1], np.int32), np.array([0], np.int32), 1, {"uniform": np.full(1, 2.5), "negative": np.full(1, -1.5)},
                     dict(m=1, n=1, col_degs={1}), err_weight=1))
    for n in (31, 32, 33):
        ip, ix = GS.deal(rng_of(f"n{n}/graph"), 12, np.full(n, 3))
        out.append(_case(f"n{n}", ip, ix, n, {"uniform": np.full(n, 4.0), "three values": GS.by_class(rng_of(f"n{n}p"), n, [-1.5, 1.7, 4.0])},
                         dict(m=12, n=n, col_degs={3}), err_weight=1))
    # ---- ties that cross every wave: more than half of the columns have degree 0, lie scattered over the index range and carry TIE_PRIOR, which no
    # other column's |V| can reach before the second decimation (|prior| + degree * alpha * max(clip_llr, |prior|) <= 4 + 3 * 20 without degree-1
    # checks).  Their marginal is 0.0 + bias for good, so with per_round = 64 a decimation takes the 64 lowest of them that are left.  Below the block
    # size there is exactly one in every stride of block / 64 columns, at a random place in it: the first 64 picks have 64 distinct owner threads,
    # eight in each of the eight waves (512 threads) or four in each of the sixteen (1024), so every wave wins picks against equal keys in all the
    # others.  Every column from the block size on is tied, so each of those owners rescans to another tied column of its own.
    for name, n, degs in (("ties_512", 1100, ((3, 448),)), ("ties_1024", 4200, ((2, 700), (1, 260)))):
        nt = block_threads(32, n)
        r = rng_of(name)
        low = np.arange(64) * (nt // 64) + r.integers(0, nt // 64, 64)
        cd = np.zeros(n, np.int64)
        cd[np.setdiff1d(np.arange(nt), low)] = GS.blocks(r, *degs)
        ip, ix = GS.deal(rng_of(name + "/graph"), 32, cd)
        prior = np.where(cd == 0, TIE_PRIOR, GS.by_class(rng_of(name + "p"), n, [-1.5, 2.5, 4.0]))
        out.append(_case(name, ip, ix, n, {"tie class": prior}, dict(m=32, n=n, col_degs={0} | {d for d, _ in degs}, ties=True, block=nt), err_weight=4))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# ---------------------------------------------------------------------------------------- the model's runs, once per case
_CASES, _SYND, _RUNS = [], {}, {}


def all_cases():
    if not _CASES:
        _CASES.extend(cases())
    return _CASES


def syndromes(c):
    if c.name not in _SYND:
        _SYND[c.name] = GS.syndromes(c, B)
    return _SYND[c.name]


def decim_reference(c, prior_name, set_name):
    """-> (the six outputs of decimation_model.decim_decode on the B syndromes of the case, its trace); computed once, shared, never changed."""
    key = (c.name, prior_name, set_name)
    if key not in _RUNS:
        trace = []
        with np.errstate(invalid="ignore"):                                 # inf - inf where two degree-1 checks disagree on a column: the NaN is meant
            ref = DM.decim_decode(c.indptr, c.indices, c.n, syndromes(c), c.priors[prior_name], trace=trace, **DECIM_SETS[set_name])
        for a in ref:
            a.setflags(write=False)
        _RUNS[key] = (ref, trace)
    return _RUNS[key]
