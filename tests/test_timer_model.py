"""The reference model of the timers (tests/timer_model.py), without a GPU: pinned to the frozen FIFO oracle
when no timer is in use, and checked against the known answers restated from the reference's TimerSpec
(tests/golden/timer_kats.json)."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import timer_cases as tc
from tests.timer_model import TimerModel, clamp_delay
from tests.test_prio_model import run_oracle as run_fifo_oracle, same


def run_model(w, max_steps=1 << 30):
    m = TimerModel(**w.engine_kwargs())
    w.apply_to(m)
    st = m.run(max_steps)
    return m, st, m.read_state(), m.take_outbound()


def run_oracle(w, max_steps=1 << 30):
    """the frozen oracle knows no timers: the workload without them"""
    saved, w.timers = w.timers, {}
    try:
        return run_fifo_oracle(w, max_steps)
    finally:
        w.timers = saved


# ------------------------------------------------------------------ pinned to the frozen oracle
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("timers", [False, True])
@pytest.mark.parametrize("mix", ["priority_mix", "compiled"])
def test_model_equals_oracle(mix, timers, T):
    """no timers, and timers set but none ever started: the frozen oracle's results"""
    w = wl.priority_mix(2048, seed=5 + T, throughput=T, tables=False) if mix == "priority_mix" else \
        wl.compiled(4096, seed=3, throughput=T)
    assert w.max_emit == 1  # (timers need it)
    w.timers = {"n_keys": 2} if timers else {}
    m, st, state, out = run_model(w)
    assert same((st, state, out), run_oracle(w)) is None
    assert m.timer_info() == dict(fired=0, discarded=0, active=0, pending=0, ticks=st["supersteps"] if timers else 0)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", tc.KAT_T)
@pytest.mark.parametrize("name", tc.KAT_NAMES)
def test_kat(name, T):
    w = tc.kat_workload(name, T)
    m = TimerModel(**w.engine_kwargs())
    w.apply_to(m)
    tc.check_kat(name, T, tc.run_kat(name, T, m))


def test_kats_restate_the_spec():
    assert set(tc.KAT_NAMES) == {"non_repeated", "repeated", "replace", "cancel", "keep_across_become", "stop_cancels"}
    for s in tc.KATS["scenarios"]:
        assert s["lines"].startswith("TimerSpec.scala:") and len(s["echo"]) == len(s["script"])


def test_replace_precedes_the_fire():
    """the Bump of `replace` is staged for the tick of a fire: the old generation's message is in the inbox behind it"""
    w = tc.kat_workload("replace", 5)
    m = TimerModel(**w.engine_kwargs())
    w.apply_to(m)
    m.run(5)
    assert m.read_timers(tc.ACTOR)["remaining"][0] == 1 and m.read_timers(tc.ACTOR)["generation"][0] == 1
    m.tell(tc.ACTOR, tc.payload("Bump"))
    m.run(1)
    assert m.timer_info()["discarded"] == 1 and m.read_timers(tc.ACTOR)["generation"][0] == 2


# ------------------------------------------------------------------ the rules the scenarios do not reach
def test_delay_clamp():
    assert [clamp_delay(d) for d in (0, 1, 7, (1 << 31) - 1, 1 << 31, (1 << 64) - 1, 1 << 63)] == \
        [1, 1, 7, (1 << 31) - 1, (1 << 31) - 1, 1, 1]


def test_bounded_mailbox_fire_is_a_dead_letter():
    """capacity 2, full at the fire: the TimerMsg dies, `fired` counts it, the single slot stays active with
    nothing to come and the engine goes quiescent"""
    w = tc.kat_workload("non_repeated", 1)  # (a single timer of delay 2 on ACTOR, throughput 1)
    w.capacity = 2
    m = TimerModel(**w.engine_kwargs())
    w.apply_to(m)
    m.tell(np.full(3, tc.ACTOR, np.uint32), np.full(3, tc.payload("Become"), np.uint32))  # tick 1: 2 admitted, 1 drained
    m.run(1)
    m.tell(tc.ACTOR, tc.payload("Become"))  # tick 2: backlog 1 + staged 1 = full; the TimerMsg is third
    st = m.run()
    info, slot = m.timer_info(), m.read_timers(tc.ACTOR)
    assert info == dict(fired=1, discarded=0, active=1, pending=0, ticks=3)
    assert slot["active"][0] == 1 and slot["remaining"][0] == 0xFFFFFFFF
    assert st["dead_letters"] == 2 and st["delivered"] == 3 and st["in_flight"] == 0
    assert st["staged"] + st["emitted"] + info["fired"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def test_heartbeat_guard():
    """the population the GPU parity test runs is not vacuous: fires, discards, cancels, stops and echoes occur"""
    for seed in (1, 2):
        w = wl.heartbeat(2048 + 37, 7, seed=seed, throughput=3, bucket_actors=128)
        m = TimerModel(**w.engine_kwargs())
        w.apply_to(m)
        m.run(3)
        st = m.run(40)
        info = m.timer_info()
        assert info["ticks"] == 43 and info["fired"] > 2048 and info["discarded"] > 0
        assert info["active"] < 2048 + 37 and (m.read_state()[1] == 0).any() and m.take_outbound()[0].size > 0
        assert st["staged"] + st["emitted"] + info["fired"] == st["delivered"] + st["dead_letters"] + st["in_flight"]
        assert m.max_bucket_inbox(128) <= 2048 and m.max_bucket_inbox(2048) <= 2048
