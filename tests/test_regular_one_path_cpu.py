"""The static shape of the bare pass of the fixed-work ownership form (csrc/minsum_regular.hip, PLACE), no GPU: what profiles/isa_mix.json records for the
headline kernel, which tests/test_kernel_sources_cpu.py keeps in step with the sources (tools/isa_mix.py --record refuses a loop that does not have exactly
one path without selects and one with eight).  A wave of class "none" runs one straight path: no select, one conditional branch besides the back-edge and
no jump, at most the 56 vector instructions r27 gave it; every other wave pays its eight selects and one jump back; nothing inside the loop touches
scratch, and the kernel keeps 64 vector registers, so eight waves share a SIMD's file as the launch bounds ask."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_common_wave_runs_one_straight_path():
    with open(os.path.join(ROOT, "profiles", "isa_mix.json")) as fh:
        e = json.load(fh)["entries"]["cc_bb144_fixed"]
    assert "minsum_regular_kernel<6, 3, false, true, true, true, true>" in e["kernel"]
    none, other = e["paths"]
    assert none["selects"] == 0 and none["branches"] == 2 and none["valu"] <= 56 and none["issue_cycles"] <= 192 and none["lds"] == 14
    assert other["selects"] == 8 and other["branches"] == 3 and other["valu"] <= 64 and other["lds"] == 14
    assert none["mix"].get("vmem", 0) == 0 and other["mix"].get("vmem", 0) == 0 and e["scratch_in_loop"] == 0
    assert none["mix"]["salu"] <= 8                                                   # the one-block loop before the arms had 7; plus the class test
    assert e["mix"] == none["mix"] and e["valu_instructions"] == none["valu"]       # bench.py prices the straight path
    assert e["code_object"]["vgpr_count"] <= 64
