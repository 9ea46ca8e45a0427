"""The header rule of csrc/ (DESIGN.md 5.3), checked on the text alone: a priced kernel's record names every file that can reach its instruction stream,
the launcher headers reach none, and the committed static instruction mix matches the tree.  No GPU, no compiler."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qldpc-branched-off_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_mix  # noqa: E402

DEVICE_MARKS = ("__device__", "__global__", "__shared__", "asm(")
HOST_ONLY = ("launchers.h", "common.h", "../../include/qldpc_hip.h")      # what the split leaves without device code, as csrc/ includes them


def read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def host_only(name):
    text = read(name)
    return not any(mark in text for mark in DEVICE_MARKS)


def include_closure(name):
    """every file `name` reaches through #include "..." inside the repository, as paths relative to csrc/ (itself included)"""
    seen, todo = set(), [name]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        todo += [os.path.normpath(os.path.join(os.path.dirname(f), inc)) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', read(f), re.M)]
    return seen


def test_launcher_headers_hold_no_device_code():
    for h in HOST_ONLY:
        assert host_only(h), f"{h} holds device code: move it to a device header (and into the file lists of tools/isa_mix.py RECORDED)"


def test_every_record_lists_what_its_kernel_includes():
    lists = {key: (v[0], v[3]) for key, v in isa_mix.RECORDED.items()}
    for key, (src, files) in lists.items():
        assert src in files
        for f in files:
            assert os.path.normpath(f) not in [os.path.normpath(h) for h in HOST_ONLY], f"{key}: {f} is a host-only header"
        unlisted = include_closure(src) - {os.path.normpath(f) for f in files}
        for f in sorted(unlisted):
            assert host_only(f), f"{key}: {src} reaches {f}, which holds device code and is not in the record's file list"
    for key, files in isa_mix.RECORDED_ALSO.items():
        assert files in [v[1] for v in lists.values()], f"{key}: not the list of a kernel of RECORDED"


def test_committed_instruction_mix_is_fresh():
    """python tools/isa_mix.py --record refreshes it, on any machine with the compiler: a change to a priced kernel's files comes with it."""
    with open(os.path.join(ROOT, "profiles", "isa_mix.json")) as fh:
        entries = json.load(fh)["entries"]
    assert set(entries) == set(isa_mix.RECORDED)
    for key, (_, kernel, _, files) in isa_mix.RECORDED.items():
        e = entries[key]
        assert e["sources"] == files, key
        assert kernel in e["kernel"], f"{key}: the record counted {e['kernel']}"
        assert e["source_digest"] == isa_mix.digest(files), f"{key}: profiles/isa_mix.json is stale -- run python tools/isa_mix.py --record"
