"""The region layout of the host-pointer entry points' staging helper (csrc/stage_layout.h: pure arithmetic, no HIP header) against a model restated
here (no GPU): a stand-alone host program (tests/host_stage_main.cpp) is compiled with the compiler the library is built with, once plainly and once
under the address and undefined-behaviour sanitizers, and both are run on every region list below."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
ALIGN, SIZE_MAX = 256, 2 ** 64 - 1


MAX_REGIONS = 24


def model(regions):
    """[(dims, elem)] -> (total, offsets), or None where a dimension is negative, a product, a byte count or the running total does not fit size_t, or
    there are more than MAX_REGIONS regions.  dims: a tuple of signed dimensions (the form the helper calls), or a bare unsigned count."""
    total, offs = 0, []
    if len(regions) > MAX_REGIONS:
        return None
    for dims, elem in regions:
        count = 1
        for d in (dims if isinstance(dims, tuple) else (dims,)):
            if d < 0 or count * d > SIZE_MAX:
                return None
            count *= d
        bytes_ = count * elem
        if bytes_ + ALIGN - 1 > SIZE_MAX:
            return None
        offs.append(total)
        total += max(-(-bytes_ // ALIGN) * ALIGN, ALIGN)           # an empty region still owns one unit: its address is its own
        if total > SIZE_MAX:
            return None
    return total or ALIGN, offs                                    # never an allocation of zero bytes


I63 = 2 ** 63 - 1
LISTS = [
    [],
    [(0, 1)],
    [(0, 8), (0, 4), (0, 1)],
    [(1, 1)],
    [(255, 1), (256, 1), (257, 1)],
    [(3, 7), (3, 8), (21, 8), (3, 4), (0, 4), (3, 1)],                         # B = 3 on the 3 x 7 Hamming matrix: no size a multiple of 256
    [(144, 8), (72, 1), (144, 8), (1, 4), (144, 1), (1, 1)],                   # one shot of [[144,12,12]]
    [(1 << 31, 8), (5, 1), ((1 << 31) + 1, 4)],                                # offsets past 2^32
    [(1, 1)] * 19,
    [(2 ** 61, 8)],                                                            # 2^64 bytes
    [(2 ** 64 - 1, 2)],
    [(3, 1), (2 ** 63, 2), (3, 1)],
    [(SIZE_MAX, 1)],                                                           # fits, but not once it is rounded up
    [(SIZE_MAX - 255, 1)],                                                     # a multiple of 256 that fits ...
    [(1, 1), (SIZE_MAX - 255, 1)],                                             # ... but not behind another region
    [(2 ** 62, 1), (2 ** 62, 1), (2 ** 62, 1), (2 ** 62, 1)],                  # each fits, the sum does not
    # the same through dimension lists, as every entry point declares its regions
    [((3, 7), 1), ((3, 7), 8), ((7,), 8), ((3,), 4), ((3, 0), 4), ((), 4), ((3, 3, 5), 8), ((2, 3, 5, 7), 2)],
    [((0, 7), 1), ((5, 0, 9), 8), ((0,), 4)],                                  # an empty batch, a matrix without rows: three addresses
    [((1 << 31, 1 << 20), 8), ((5,), 1)],                                      # int64 x int products beyond 2^32 that fit
    [((1 << 32, 1 << 32), 1)],                                                 # the product of the dimensions is 2^64 ...
    [((1 << 31, 1 << 31, 4), 1)],
    [((1 << 31, 1 << 30), 8)],                                                 # ... the element count fits, its bytes do not
    [((I63, 2), 1), ((1,), 1)],                                                # 2^64 - 2 elements fit, not once rounded up
    [((3,), 1), ((-1,), 1)],                                                   # negative dimensions: what a wrapped int64 x int product was
    [((3, -7), 8)],
    [((-3, -7), 8)],                                                           # two negatives do not make a count
    [((0, -1), 8)],                                                            # not even an empty one
    [((-(2 ** 63),), 1)],
    [((1,), 1)] * MAX_REGIONS,                                                 # the layout holds this many regions ...
    [((1,), 1)] * (MAX_REGIONS + 1),                                           # ... and refuses one more
]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def library_layout(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_stage") / ("host_stage_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", *extra, "-I", CSRC, os.path.join(HERE, "host_stage_main.cpp"), "-o", exe], check=True)

    def ask(lists):
        one = lambda dims, elem: ("%d %s %d" % (len(dims), " ".join(map(str, dims)), elem)) if isinstance(dims, tuple) else "-1 %d %d" % (dims, elem)  # noqa: E731
        text = "".join("%d %s\n" % (len(rs), " ".join(one(*r) for r in rs)) for rs in lists)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lists)
        return [None if ln == "invalid" else (int(ln.split()[1]), [int(x) for x in ln.split()[2:]]) for ln in out]
    return ask


def test_layout_equals_the_model(library_layout):
    got = library_layout(LISTS)
    for rs, g in zip(LISTS, got):
        assert g == model(rs), (rs, g, model(rs))
    assert sum(g is None for g in got) >= 16 and sum(g is not None for g in got) >= 13


def test_regions_are_aligned_disjoint_and_inside_the_allocation(library_layout):
    ok = [rs for rs in LISTS if model(rs) is not None]
    for rs, (total, offs) in zip(ok, library_layout(ok)):
        assert total >= 1 and len(offs) == len(rs)
        assert all(o % ALIGN == 0 for o in offs), rs
        assert len(set(offs)) == len(offs), rs                                 # zero-byte regions included: every region has an address of its own
        size = lambda dims, e: int(np.prod([int(d) for d in (dims if isinstance(dims, tuple) else (dims,))], dtype=object)) * e   # noqa: E731
        spans = sorted((o, o + size(*r)) for o, r in zip(offs, rs))
        assert all(a_end <= b_off for (_, a_end), (b_off, _) in zip(spans, spans[1:])), rs
        assert all(o < total for o in offs) and all(end <= total for _, end in spans), rs


def test_overflowing_byte_counts_are_rejected(library_layout):
    bad = [rs for rs in LISTS if model(rs) is None]
    assert len(bad) >= 16
    assert library_layout(bad) == [None] * len(bad)
