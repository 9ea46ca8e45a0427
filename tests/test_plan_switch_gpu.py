"""The circuit plan's switch rules as one table: every decode switch qldpc_circuit_plan_use_* (all ten) on a fresh plan, every ordered pair of them and every one applied
twice, on circ72 with batch 64.  An accepted switch leaves a plan that runs; a refused one answers QLDPC_ERR_INVALID, names the plan's state before
the requested one, and leaves the plan decoding exactly as before.  Then the two creation arguments the rules read: use_osd = 0 and damping != 1."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_relay_gpu import circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 64

def _tables(which):
    """the erasure tables or the gaussian soft tables of circ72, from the feature modules' setup (imported late: they import this module)"""
    from qldpc_amd import _lib
    if which == "erasure":
        import test_erasure_gpu
        return test_erasure_gpu.setup(_lib)[9]
    import test_soft_gpu
    return test_soft_gpu.setup(_lib)[9]["gaussian"]


# switch -> (display name in the library's messages, the call, the call with other arguments for a re-application)
BASE_SWITCHES = {
    "relay": ("Relay-BP", lambda p: p.use_relay(), lambda p: p.use_relay(t0=40, max_legs=100)),
    "osd_cs": ("BP + OSD-CS", lambda p: p.use_osd_cs(5), lambda p: p.use_osd_cs(3)),
    "window": ("sliding-window decoding", lambda p: p.use_window(4, 2), lambda p: p.use_window(3, 1)),
    "layered": ("the layered schedule", lambda p: p.use_layered(), lambda p: p.use_layered(np.arange(p.graph_z.m), None)),
    "decimation": ("guided decimation", lambda p: p.use_decimation(), lambda p: p.use_decimation(per_round=4)),
    "f32": ("single precision (f32)", lambda p: p.use_f32(), lambda p: p.use_f32()),
}
# ... and the four that came later.  The feature modules build their "new row and column" tests on BASE_SWITCHES, as they did when they were written.
SWITCHES = dict(
    BASE_SWITCHES,
    lsd=("BP + LSD", lambda p: p.use_lsd(), lambda p: p.use_lsd(max_rows=128)),
    correlated=("correlated decoding", lambda p: p.use_correlated(), lambda p: p.use_correlated(0.875)),
    erasure_aware=("erasure-aware decoding", lambda p: p.use_erasure_aware(1.0, _tables("erasure")), lambda p: p.use_erasure_aware(0.875, _tables("erasure"))),
    soft_aware=("soft-aware decoding", lambda p: p.use_soft_aware(1.0, _tables("soft")), lambda p: p.use_soft_aware(0.875, _tables("soft"))),
)

# ACCEPTED[first] = the switches a plan takes after `first` (every switch is accepted on a fresh plan); everything else is refused.
# Two axes: the path (relay, window, layered, decimation, f32, correlated, erasure_aware, soft_aware: left at most once, re-applied except window) and
# the OSD stage (osd_cs, lsd: each goes with layered, decimation, f32, correlated, erasure_aware and soft_aware in either order, with neither relay nor
# window, and they refuse each other).
STAGE_SWITCHES = ("osd_cs", "lsd")
WITH_A_STAGE = ("layered", "decimation", "f32", "correlated", "erasure_aware", "soft_aware")
ACCEPTED = {"relay": {"relay"}, "window": set()}
ACCEPTED.update({path: {path, *STAGE_SWITCHES} for path in WITH_A_STAGE})
ACCEPTED.update({stage: {stage, *WITH_A_STAGE} for stage in STAGE_SWITCHES})
assert set(ACCEPTED) == set(SWITCHES) and ACCEPTED["osd_cs"] == {"osd_cs", "layered", "decimation", "f32", "correlated", "erasure_aware", "soft_aware"}
assert all(ACCEPTED[k] == {k, "osd_cs", "lsd"} for k in ("layered", "decimation", "f32"))


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def run64(L, p):
    p.run(7, 0, BATCH)
    tally = p.read(clear=True)
    assert tally[L.TALLY["trials"]] == BATCH
    return tally


def refused(L, p, call, current, requested, reason=None):
    """`call` answers QLDPC_ERR_INVALID with `current` before `requested` in the message, and the plan decodes the same trials as before."""
    before = run64(L, p)
    with pytest.raises(L.QldpcError) as ei:
        call(p)
    msg = str(ei.value)
    assert "error -1" in msg, msg
    assert current in msg and requested in msg and msg.index(current) < msg.rindex(requested), msg
    if reason is not None:
        assert reason in msg, msg
    assert np.array_equal(run64(L, p), before), (current, requested)


def test_every_switch_on_a_fresh_plan(L):
    plan = circuit_setup(L, "circ72")[6]
    for name, (_, call, _) in SWITCHES.items():
        p = plan(batch=BATCH)
        call(p)
        run64(L, p)
        p.close()


@pytest.mark.parametrize("first", list(SWITCHES))
def test_every_ordered_pair(L, first):
    plan = circuit_setup(L, "circ72")[6]
    current, call, _ = SWITCHES[first]
    for second, (requested, call2, again) in SWITCHES.items():
        p = plan(batch=BATCH)
        call(p)
        if second in ACCEPTED[first]:
            (again if second == first else call2)(p)
            run64(L, p)
        else:
            refused(L, p, again if second == first else call2, current, requested)
        p.close()


def test_a_plan_without_osd_stage(L):
    plan = circuit_setup(L, "circ72")[6]
    for name, (requested, call, _) in SWITCHES.items():
        p = plan(batch=BATCH, use_osd=False)
        if name in ("osd_cs", "window", "lsd"):
            refused(L, p, call, "use_osd = 0", requested, reason="OSD stage")
        else:
            call(p)
            run64(L, p)
        p.close()


def test_a_damped_plan(L):
    plan = circuit_setup(L, "circ72")[6]
    for name, (requested, call, _) in SWITCHES.items():
        p = plan(batch=BATCH, damping=0.5)
        if name in ("relay", "osd_cs", "lsd"):                             # none of them reads the damping: only their own argument checks apply
            call(p)
            run64(L, p)
        else:
            refused(L, p, call, requested, "damping = 1", reason="damping")
        p.close()
