"""Every refusal of the ask pattern (agx_set_ask), by status and full text."""
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
B = typed.Behaviors


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def engine(n=80, **cfg):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, throughput=4, bucket_actors=32), **cfg)))


def asking_tables(key_first=None):
    """one behaviour whose only actions are an ask's ARM and SEND, on key 0 or (with a timer key before it) key 1: the
    message 1 makes an actor ask the actor in its word 1 (actor 0, which never answers)"""
    st = typed.State("count", "server")

    def build(timers):
        if key_first is not None:
            timers.cancel(key_first)
        return (typed.ReceiveBuilder.create(st)
                .on_message_equals(1, lambda m, s: [typed.context.ask(s.server.ref, 7, 3, on_timeout=2), B.same])
                .on_any_message(lambda m, s: [B.same]).build("asker"))
    tb = typed.compile_behaviors([B.with_timers(build)], max_emit=1)
    assert [a.op for a in tb.acts[:tb.n_acts]] == [typed.A_ASK_ARM, typed.A_ASK_SEND]
    return tb


def test_needs_timers_first(built):
    eng = engine()
    assert status_and_text(eng.set_ask) == (EINVAL, "the ask pattern needs an engine with timers (agx_set_timers first)")
    eng.close()


def test_inherits_the_timers_refusals(built):
    eng = engine(max_emit=2)  # (timers need max_emit = 1: no timers, so no ask)
    assert status_and_text(lambda: eng.set_timers(2))[0] == EINVAL
    assert status_and_text(eng.set_ask) == (EINVAL, "the ask pattern needs an engine with timers (agx_set_timers first)")
    eng.close()
    eng = engine()
    eng.set_timers(2)
    eng.set_ask()
    assert status_and_text(lambda: eng.set_death_watch(1)) == (EINVAL, "death watch needs an engine without timers (agx_set_timers)")
    assert status_and_text(lambda: eng.set_timers(3)) == \
        (EINVAL, "timers: the key count cannot change once the ask pattern is set (agx_set_ask)")
    eng.close()


def test_once_and_before_the_first_run(built):
    eng = engine()
    eng.set_timers(2)
    eng.set_ask()
    assert status_and_text(eng.set_ask) == (EINVAL, "the ask pattern is set already (agx_set_ask is called once)")
    eng.close()
    eng = engine()
    eng.register_range(0, 80, 1)
    eng.set_timers(2)
    eng.run(1)
    assert status_and_text(eng.set_ask) == (ESTATE, "set the ask pattern before the first agx_run")
    eng.close()


def test_not_with_receive_timeouts_in_either_order(built):
    eng = engine()
    eng.set_timers(1)
    eng.set_receive_timeout()
    assert status_and_text(eng.set_ask) == \
        (EINVAL, "the ask pattern needs an engine without receive timeouts (agx_set_receive_timeout): the two are features "
                 "of their own on top of the timers")
    eng.close()
    eng = engine()
    eng.set_timers(1)
    eng.set_ask()
    assert status_and_text(eng.set_receive_timeout) == \
        (EINVAL, "receive timeouts need an engine without the ask pattern (agx_set_ask): the two are features of their own "
                 "on top of the timers")
    eng.close()


def test_too_many_actors_for_the_ref(built):
    eng = engine(1 << 22, bucket_actors=2048)
    eng.set_timers(1)
    assert status_and_text(eng.set_ask) == \
        (EINVAL, "the ask pattern needs an engine of at most 4194303 actors (it has 4194304): an ask ref carries the asker's "
                 "id in 22 bits")
    eng.close()


def test_host_tells_with_a_ref_as_sender_and_outbound_ranges(built):
    eng = engine()
    eng.register_range(0, 80, 1)
    eng.set_timers(1)
    eng.set_ask()
    ref = 0x80000005
    assert status_and_text(lambda: eng.tell([3], [1], [ref])) == \
        (EINVAL, f"tell 0: sender {ref} is not an actor id (bit 31 tags CRDT state gossips)")
    assert status_and_text(lambda: eng.tell_one(3, 1, ref)) == \
        (EINVAL, f"tell: sender {ref} is not an actor id (bit 31 tags CRDT state gossips)")
    eng.tell([3], [1], [NO_SENDER])  # (no sender is fine)
    assert status_and_text(lambda: eng.set_outbound((1 << 31) - 4, 8)) == \
        (EINVAL, "host ids must lie in [n_actors, 2^31) (bit 31 of a sender tags CRDT state gossips)")
    eng.close()


def test_tables_that_ask_on_an_engine_without_ask(built):
    tb = asking_tables()
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_timers(1)
    eng.tell([3], [1])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours ask, but the engine has no ask pattern (agx_set_ask)")
    eng.set_ask()  # (then it runs)
    st = eng.run()
    assert eng.ask_info() == dict(asked=1, answered=0, timed_out=1, late=0) and st.in_flight == 0
    eng.close()


def test_half_an_ask(built):
    for half in ("send_of_another_key", "arm_alone", "send_alone"):
        tb = asking_tables()
        if half == "send_of_another_key":
            tb.acts[1].word = 1
        elif half == "arm_alone":
            tb.acts[1].op = typed.A_SET
            tb.acts[1].word = 0
        else:
            tb.acts[0].op = typed.A_SET
        eng = engine()
        eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
        eng.set_behaviors(tb)
        eng.set_timers(2)
        eng.set_ask()
        eng.tell([3], [1])
        assert status_and_text(lambda: eng.run(1)) == \
            (EINVAL, f"the compiled behaviours' action {1 if half == 'send_alone' else 0} is half an ask: AGX_A_ASK_SEND comes "
                     "directly after the AGX_A_ASK_ARM of the same key"), half
        eng.close()


def test_an_ask_key_past_n_keys(built):
    tb = asking_tables(key_first="a timer's")
    assert tb.acts[0].word == 1
    eng = engine()
    eng.register_range(0, 80, tb.kind_of(tb.behaviors[0]))
    eng.set_behaviors(tb)
    eng.set_timers(1)
    eng.set_ask()
    eng.tell([3], [1])
    assert status_and_text(lambda: eng.run(1)) == \
        (EINVAL, "the compiled behaviours ask on timer key 1, but the engine has 1 slots per actor (agx_set_timers)")
    eng.close()


def test_a_constant_timeout_below_one_in_the_tables(built):
    tb = asking_tables()
    tb.acts[0].dk = 0
    eng = engine()
    assert status_and_text(lambda: eng.set_behaviors(tb)) == \
        (EINVAL, "compiled behaviours: action 0 asks with a timeout of 0 ticks (a constant timeout is at least 1)")
    eng.close()
