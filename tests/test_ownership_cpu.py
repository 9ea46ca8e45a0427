"""Who frees what, checked without a GPU.  On the text of csrc/: device and pinned memory are allocated and freed in one owning type each,
and the hand-kept release lists are gone.  On the Python mirror: the header declares the live-allocation count and the binding carries it, and the wrapper
base destroys a handle exactly once."""
import ctypes as C
import glob
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "qldpc-branched-off_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def read(path):
    with open(path) as fh:
        return fh.read()


def function_body(text, signature):
    """the text of the top-level function whose definition starts with `signature`, up to its closing brace in column 0"""
    start = text.index(signature)
    return text[start:text.index("\n}", start) + 2]


def calls_outside(names, allowed):
    """{file: count} of calls of `names` outside the function bodies `allowed` = {file name: [signatures]}"""
    out = {}
    for path in SOURCES:
        text, name = read(path), os.path.basename(path)
        for sig in allowed.get(name, []):
            text = text.replace(function_body(text, sig), "")
        n = sum(text.count(call) for call in names)
        if n:
            out[name] = n
    return out


def test_sources_are_found():
    assert len(SOURCES) >= 40 and os.path.join(CSRC, "graph.hip") in SOURCES


def test_device_memory_is_allocated_and_freed_in_devbuf_alone():
    allowed = {"graph.hip": ["int DevBuf::ensure(size_t bytes) {", "void DevBuf::release() {"],
               "gf2.hip": ["unsigned long long *osd_timer_buffer() {"]}          # process lifetime: the diagnostic build's timer buffer
    for sigs, name in ((allowed["graph.hip"], "graph.hip"), (allowed["gf2.hip"], "gf2.hip")):
        for sig in sigs:
            body = function_body(read(os.path.join(CSRC, name)), sig)
            assert "hipMalloc(" in body or "hipFree(" in body, f"{sig} no longer allocates or frees: update this test"
    assert calls_outside(("hipMalloc(", "hipFree("), allowed) == {}


def test_pinned_memory_is_allocated_and_freed_in_its_owner_alone():
    allowed = {"graph.hip": ["int PinnedBuf::ensure(size_t bytes) {", "void PinnedBuf::release() {"]}
    text = read(os.path.join(CSRC, "graph.hip"))
    assert "hipHostMalloc(" in function_body(text, allowed["graph.hip"][0]) and "hipHostFree(" in function_body(text, allowed["graph.hip"][1])
    assert calls_outside(("hipHostMalloc(", "hipHostFree("), allowed) == {}


def test_release_lists_and_the_plan_buffer_type_are_gone():
    for path in SOURCES:
        text, name = read(path), os.path.basename(path)
        assert "PlanBuf" not in text, name
        if name != "minsum_wg2.hip":             # keeps its list (its text is pinned by the recorded instruction mix); harmless: release() is idempotent
            assert not re.search(r"\bb\s*->\s*release\s*\(\s*\)", text), name
            assert "hand.destroy()" not in text, name
    common = read(os.path.join(CSRC, "common.h"))
    devbuf = common[common.index("struct DevBuf {"):common.index("};", common.index("struct DevBuf {"))]
    assert "~DevBuf()" in devbuf and "DevBuf(const DevBuf &) = delete;" in devbuf and "DevBuf(DevBuf &&o)" in devbuf
    # one upload helper: the template of common.h (minsum_wg2.hip keeps its private copy under another name)
    defs = [os.path.basename(p) for p in SOURCES if re.search(r"^(static )?int (upload|up)\(", read(p), re.M)]
    assert sorted(defs) == ["common.h", "minsum_wg2.hip"], defs


def test_header_declares_the_count_and_the_binding_carries_it():
    from qldpc_amd import _lib
    header = read(os.path.join(ROOT, "include", "qldpc_hip.h"))
    assert re.search(r"\bint\s+qldpc_device_memory\s*\(\s*int64_t\s*\*\s*buffers\s*,\s*int64_t\s*\*\s*bytes\s*\)\s*;", header)
    restype, argtypes = _lib.signatures()["qldpc_device_memory"]
    assert restype is C.c_int and argtypes == [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert callable(_lib.device_memory)
    assert 'QLDPC_EXPORT int qldpc_device_memory(' in read(os.path.join(CSRC, "graph.hip"))


class FakeLib:
    """stands in for the loaded library: records every destroy call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("qldpc_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))


@pytest.fixture
def fake(monkeypatch):
    from qldpc_amd import _lib
    f = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: f)
    return _lib, f


OWNERS = ("Graph", "WindowDecoder", "LayeredDecoder", "Minsum32Decoder", "Comm", "CodeCapacityPlan", "MessageStats", "CircuitPlan", "DemPlan", "Stream")


@pytest.mark.parametrize("cls", OWNERS)
def test_wrapper_base_destroys_once(fake, cls):
    L, f = fake
    T = getattr(L, cls)
    assert issubclass(T, L.Owner) and isinstance(T._destroy, str) and T._destroy in L.signatures()
    o = T.__new__(T)                             # no create call: the base must cope with a wrapper whose __init__ never ran
    o.close()
    o.__del__()
    assert f.calls == []
    o._h, o.device = C.c_void_p(0x1234), 3
    assert o.handle is o._h
    o.close()
    want = (T._destroy, (3, 0x1234) if cls == "Stream" else (0x1234,))
    assert f.calls == [want]
    assert not o._h.value                         # `_h` stays a c_void_p (NULL), so a later call fails in the library's NULL check, not in ctypes
    o.close()
    o.__del__()
    assert f.calls == [want]
    o2 = T.__new__(T)
    o2._h, o2.device = C.c_void_p(0x99), 0
    o2.__del__()                                  # without close(): __del__ destroys
    o2.__del__()
    assert len(f.calls) == 2 and f.calls[1][0] == T._destroy


def test_wrapper_classes_spell_out_no_close_of_their_own(fake):
    L, _ = fake
    for cls in OWNERS:
        T = getattr(L, cls)
        for name in ("close", "__del__", "handle"):
            assert name not in vars(T), f"{cls}.{name} shadows the base"


def test_prior_check_texts(fake):
    L, _ = fake
    with pytest.raises(ValueError, match=r"^prior has 3 entries, H has 4 columns$"):
        L.prior_of([1.0, 2.0, 3.0], 4)
    with pytest.raises(ValueError, match=r"^initialBelief has 3 entries, H has 4 columns$"):
        L.prior_of([1.0, 2.0, 3.0], 4, "initialBelief")
    with pytest.raises(ValueError, match=r"^prior has 3 entries, the graph has 4 columns$"):
        L.prior_of([1.0, 2.0, 3.0], 4, owner="the graph")
    p = L.prior_of([[1, 2], [3, 4]], 4)
    assert p.dtype.name == "float64" and p.shape == (4,) and p.flags["C_CONTIGUOUS"]
