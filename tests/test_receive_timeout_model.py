"""The reference model of the receive timeouts (tests/receive_timeout_model.py), without a GPU: with no timeout set
it equals the timers' model on the timers' own scenarios (so it stays pinned to the frozen oracle through
tests/test_timer_model.py), and it satisfies the known answers restated from the reference's ReceiveTimeoutSpec and
ActorContextSpec (tests/golden/receive_timeout_kats.json)."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import receive_timeout_cases as rc
from tests import timer_cases as tc
from tests.receive_timeout_model import ReceiveTimeoutModel
from tests.test_prio_model import same
from tests.timer_model import TimerModel


def model_for(w):
    m = ReceiveTimeoutModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


# ------------------------------------------------------------------ with no timeout set: the timers' model
@pytest.mark.parametrize("T", tc.KAT_T)
@pytest.mark.parametrize("enabled", [False, True])
@pytest.mark.parametrize("name", tc.KAT_NAMES)
def test_equals_the_timer_model_on_the_timer_kats(name, enabled, T):
    """the timers' known answers, on the model without and with receive timeouts enabled (none ever set)"""
    w = tc.kat_workload(name, T)
    if enabled:
        w.timers = dict(w.timers, receive_timeout={"transparent": (1, 3)})
    m = model_for(w)
    got = tc.run_kat(name, T, m)
    tc.check_kat(name, T, got)
    t = TimerModel(**w.engine_kwargs())
    w.timers.pop("receive_timeout", None)
    w.apply_to(t)
    assert got == tc.run_kat(name, T, t)
    assert m.receive_timeout_info() == dict(fired=0, discarded=0, set=0, pending=0)


@pytest.mark.parametrize("T", [1, 3])
def test_equals_the_timer_model_on_heartbeats(T):
    w = wl.heartbeat(300, 7, seed=3, throughput=T, bucket_actors=32)
    t = TimerModel(**w.engine_kwargs())
    w.apply_to(t)
    w.timers = dict(w.timers, receive_timeout={})
    m = model_for(w)
    for budget in (3, 30):
        assert same((m.run(budget), m.read_state(), m.take_outbound()), (t.run(budget), t.read_state(), t.take_outbound())) is None
    assert m.timer_info() == t.timer_info() and m.timer_info()["fired"] > 300
    assert all(np.array_equal(m.read_timers(a)[k], t.read_timers(a)[k]) for a in range(300) for k in ("active", "remaining"))


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", rc.KAT_T)
@pytest.mark.parametrize("name", rc.KAT_NAMES)
def test_kat(name, T):
    rc.check_kat(name, T, rc.run_kat(name, T, model_for(rc.kat_workload(name, T))))


def test_kats_restate_the_specs():
    lines = [s["lines"] for s in rc.KATS["scenarios"]]
    for want in ("63-76", "78-94", "96-117", "119-130", "132-152", "154-170", "172-194", "196-210", "212-228", "230-247",
                 "249-278"):
        assert "ReceiveTimeoutSpec.scala:" + want in lines
    assert [x for x in lines if x.startswith("ActorContextSpec.scala:")] == ["ActorContextSpec.scala:565-586",
                                                                              "ActorContextSpec.scala:587-610"]
    for s in rc.KATS["scenarios"]:
        assert len(rc.per_T(s["echo"], 1)) == len(s["script"]) == len(rc.per_T(s["ticks"], 5))


# ------------------------------------------------------------------ the rules the scenarios do not reach
def test_stale_envelope_carries_the_replaced_message():
    """an envelope enqueued behind a SetTimeout is delivered with the message stored at receipt: no generation"""
    w = rc.kat_workload("typed_large_timeout", 1)
    m = model_for(w)
    m.start_receive_timeout(rc.ACTOR, 1, 1, rc.payload("Ping"))   # fires at tick 1, behind the staged SetTimeout
    m.tell(rc.ACTOR, rc.payload("SetTimeout:50"))
    m.run(2)
    assert m.take_outbound()[2].tolist() == [rc.payload("TimeoutSet"), rc.payload("GotTimeout")]
    assert m.receive_timeout_info() == dict(fired=1, discarded=0, set=1, pending=1)
    assert int(m.read_receive_timeout(rc.ACTOR, 1)["remaining"][0]) == 50


def test_envelope_discarded_after_a_cancel():
    w = rc.kat_workload("turn_off_in_transparent_handler", 1)
    m = model_for(w)
    m.start_receive_timeout(rc.ACTOR, 1, 1, rc.payload("Timeout"))
    m.tell(rc.ACTOR, rc.payload("TransparentTick"))   # tick 1: the cancel; the envelope of tick 1 is behind it
    st = m.run()
    assert m.receive_timeout_info() == dict(fired=1, discarded=1, set=0, pending=0)
    assert st["delivered"] == 2 and st["unhandled"] == 0 and m.timer_info()["ticks"] == 2 and m.take_outbound()[2].size == 0


def test_passivating_entities_guard():
    """the population the GPU test runs is not vacuous: every entity passivates once, and the run goes quiescent"""
    w = wl.passivating_entities(96, 3, idle=3)
    m = model_for(w)
    st = w.run_schedule(m)
    words, alive = m.read_state()
    info = m.receive_timeout_info()
    assert not alive[:96].any() and alive[96:].all() and int(words[96:, 0].sum()) == info["fired"] >= 96
    assert int(words[:96, 0].sum()) == sum(len(d) for d, _, _ in w.schedule) and st["in_flight"] == 0
    assert {k: info[k] for k in ("discarded", "set", "pending")} == dict(discarded=0, set=0, pending=0)
    assert m.max_bucket_inbox(32) <= 2048
    assert rc.conserved(st, m.timer_info(), m.receive_timeout_info())
