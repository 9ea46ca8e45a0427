"""The pairs of tests/test_plan_pairs_gpu.py are the accepted set of switch_allowed (csrc/circuit.hip), restated as plan_pairs.allowed: every path but
Relay-BP and windows, crossed with LSD, and with a confidence on top.  The refused pairs are the ones the feature modules refuse, the switch table of
tests/test_plan_switch_gpu.py states the same rule, and include/qldpc_hip.h names every path at qldpc_circuit_plan_use_lsd.  No GPU."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_pairs as PP  # noqa: E402


def source(*parts):
    with open(os.path.join(HERE, *parts)) as f:
        return f.read()


def test_the_predicate_states_the_rule():
    for path in PP.PATHS:
        assert PP.allowed(path, "osd0") and not PP.allowed(path, "osd0", confidence=True)
        for stage in ("osd_cs", "lsd"):
            assert PP.allowed(path, stage) == (path not in ("relay", "window"))
            assert not PP.allowed(path, stage, use_osd=False)
        assert PP.allowed(path, "osd0", use_osd=False) == (path != "window")
        assert PP.allowed(path, "osd0", damping=0.5) == (path in ("flooding", "relay"))
        assert PP.allowed(path, "lsd", damping=0.5) == (path == "flooding")
        assert PP.allowed(path, "lsd", confidence=True) == PP.allowed(path, "lsd") and not PP.allowed(path, "osd_cs", confidence=True)


def test_the_gpu_cases_are_the_accepted_set():
    accepted = [path for path in PP.PATHS if PP.allowed(path, "lsd") and PP.allowed(path, "lsd", confidence=True)]
    refused = [path for path in PP.PATHS if not PP.allowed(path, "lsd")]
    assert refused == list(PP.WITHOUT_STAGE_SWITCH) == ["relay", "window"]
    assert sorted({PP.path_of(case) for case in PP.ALL_CASES}) == sorted(accepted)
    assert PP.ALL_CASES[0] == "flooding" and PP.LSD_CASES == PP.ALL_CASES[1:] and len(PP.LSD_CASES) == 7
    assert [c for c in PP.LSD_CASES if c.startswith("correlated")] == ["correlated:raise", "correlated:condition"]
    assert set(PP.ALPHA) == {c for c in PP.ALL_CASES if PP.path_of(c) in ("correlated", "erasure_aware", "soft_aware")}
    assert set(PP.KINDS) <= set(PP.SM.KINDS) and {PP.SM.KINDS.index(k) % 3 for k in PP.KINDS} == {0, 1, 2}      # a sum, a sum of squares, a max
    gpu = source("test_plan_pairs_gpu.py")
    for test in ("test_lsd_behind_each_path", "test_confidence_behind_each_path", "test_events_door"):
        assert re.search(r'parametrize\("case", PP\.ALL_CASES\)\ndef ' + test, gpu), test
    assert re.search(r"CASES = \{\n(    \"[a-z_:0-9]+\": dict\(.*\n)+\}", gpu)
    cases = re.findall(r'^    "([a-z_:0-9]+)": dict\(shape=', gpu, re.M)
    assert cases == list(PP.ALL_CASES)


def test_the_refused_pairs_are_the_ones_the_feature_modules_refuse():
    lsd = source("test_lsd_gpu.py")
    for first, match in (("p.use_relay()", '"Relay-BP"'), ("p.use_window(3, 1)", '"sliding-window"'), ("p.use_osd_cs(7)", '"BP \\\\+ OSD-CS: BP \\\\+ LSD cannot follow"')):
        assert f"    {first}\n    refused(p, lambda p: p.use_lsd(), {match})" in lsd, first
    assert 'refused(plan(batch=256, use_osd=False), conf, "use_osd = 0")' in source("test_lsd_stats_gpu.py")
    for module in ("test_correlated_gpu.py", "test_erasure_gpu.py", "test_soft_gpu.py"):              # each new path goes with OSD-CS and LSD, and with nothing else
        assert 'GOES_WITH = {"osd_cs", "lsd"}' in source(module), module


def test_the_switch_table_is_the_same_rule():
    import test_plan_switch_gpu as TS                                      # (imports nothing that needs a device)
    name = {"osd_cs": "osd_cs", "lsd": "lsd"}
    assert len(TS.SWITCHES) == 10 and set(TS.SWITCHES) - set(name) == set(PP.PATHS) - {"flooding"}
    assert list(TS.BASE_SWITCHES) == ["relay", "osd_cs", "window", "layered", "decimation", "f32"]
    for first in TS.SWITCHES:
        for second in TS.SWITCHES:
            if first in name and second in name:
                want = first == second                                     # OSD-CS and LSD refuse each other; either may be asked for again
            elif first in name or second in name:
                want = PP.allowed(second if first in name else first, name.get(first) or name[second])
            else:
                want = first == second and first != "window"               # a plan leaves flooding once; windows cannot be asked for again
            assert (second in TS.ACCEPTED[first]) == want, (first, second)
    for key, (display, _, _) in TS.SWITCHES.items():
        if key not in name and key not in ("f32", "window"):
            assert display == PP.PATH_NAMES[key], key


def test_the_header_names_every_path_at_use_lsd():
    header = source("..", "include", "qldpc_hip.h")
    end = header.index("int qldpc_circuit_plan_use_lsd(")
    comment = " ".join(header[header.rindex("/*", 0, end):end].split())
    comment = comment.replace(" * ", " ")
    for case in PP.LSD_CASES:
        assert PP.PATH_NAMES[PP.path_of(case)] in comment, case
    assert "flooding" in comment and "Relay-BP" in comment and "windows" in comment and "OSD-CS" in comment
    assert comment.index("goes with") < comment.index(PP.PATH_NAMES["soft_aware"]) < comment.index("QLDPC_ERR_INVALID")
