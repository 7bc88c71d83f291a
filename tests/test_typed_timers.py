"""Behaviors.with_timers in the typed DSL (akka_amd/typed.py): the lowering of every TimerScheduler call, the
mapping of keys to slots, the setup starts, and what is refused at compile time."""
import pytest

from akka_amd import typed
from akka_amd.typed import Behaviors as B

ST = typed.State("a", "b")
TICK = typed.MessageType("Tick", 1)


def lower(handler, test=None):
    def build(timers):
        return typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: handler(timers, m, s), test=test).build("t")
    b = B.with_timers(build)
    return b, typed.compile_behaviors([b], max_emit=1)


def test_start_single():
    b, t = lower(lambda tm, m, s: [tm.start_single_timer("k", TICK(7), 3), B.same])
    a = t.acts[0]
    assert (a.op, a.word, a.src, a.k, a.or_mask, a.dsrc, a.dk) == (typed.A_TIMER_SINGLE, 0, typed.V_CONST, 7, 1 << 24,
                                                                 typed.V_CONST, 3)
    assert t.timer_keys == 1 and t.initial_timers == []


def test_periodic_names_coincide():
    _, t1 = lower(lambda tm, m, s: [tm.start_timer_with_fixed_delay("k", TICK(s.a), m.arg + 1), B.same])
    _, t2 = lower(lambda tm, m, s: [tm.start_timer_at_fixed_rate("k", TICK(s.a), m.arg + 1), B.same])
    a, c = t1.acts[0], t2.acts[0]
    assert bytes(a) == bytes(c)
    assert (a.op, a.src, a.sword, a.dsrc, a.dk) == (typed.A_TIMER_PERIODIC, typed.V_WORD, 0, typed.V_ARG, 1)


def test_cancel_cancel_all_and_order():
    _, t = lower(lambda tm, m, s: [tm.start_single_timer("x", 5, 1), tm.cancel("y"), s.a.inc(), tm.cancel_all(), B.same])
    assert [t.acts[i].op for i in range(4)] == [typed.A_TIMER_SINGLE, typed.A_TIMER_CANCEL, typed.A_ADD,
                                                typed.A_TIMER_CANCEL_ALL]
    assert t.acts[0].word == 0 and t.acts[1].word == 1 and t.timer_keys == 2
    assert t.acts[0].or_mask == 0 and t.acts[0].k == 5  # a plain payload


def test_is_timer_active_is_a_test():
    def build(timers):
        timers.cancel("first")  # (key 0)
        return (typed.ReceiveBuilder.create(ST)
                .on_any_message(lambda m, s: [s.a.inc(), B.same], when=lambda m, s: timers.is_timer_active("second"))
                .build("t"))
    t = typed.compile_behaviors([B.with_timers(build)])
    c = t.cases[0]
    assert (c.src1, c.word1, c.cmp1, c.src2, c.k2) == (typed.V_TIMER, 1, typed.CMP_EQ, typed.V_CONST, 1)
    assert t.timer_keys == 2


def test_keys_map_in_order_of_appearance():
    ts = typed.TimerScheduler()
    assert [ts.cancel(k).word for k in ("b", "a", "b", ("tuple", 1), "a")] == [0, 1, 0, 2, 1]


def test_initial_timers():
    def build(timers):
        timers.start_timer_with_fixed_delay("hb", TICK(4), 16)
        timers.start_single_timer("once", 9, 2)
        return (typed.ReceiveBuilder.create(ST)
                .on_any_message(lambda m, s: [timers.start_single_timer("once", TICK(1), 5), B.same]).build("t"))
    b = B.with_timers(build)
    t = typed.compile_behaviors([b])
    k = t.kind_of(b)
    assert t.initial_timers == [(k, 0, True, 16, (1 << 24) | 4), (k, 1, False, 2, 9)]
    assert t.timer_keys == 2 and t.acts[0].op == typed.A_TIMER_SINGLE and t.acts[0].word == 1


def test_no_timers_no_keys():
    b = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [s.a.inc(), B.same]).build("plain")
    t = typed.compile_behaviors([b])
    assert t.timer_keys == 0 and t.initial_timers == []


@pytest.mark.parametrize("delay", [0, -3])
def test_constant_delay_below_one(delay):
    with pytest.raises(typed.CompileError):
        lower(lambda tm, m, s: [tm.start_single_timer("k", 1, delay), B.same])


def test_computed_delay_is_not_refused():
    lower(lambda tm, m, s: [tm.start_single_timer("k", 1, m.arg - 5), B.same])  # (below 1 counts as 1 at run time)


def test_more_than_four_keys():
    with pytest.raises(typed.CompileError):
        lower(lambda tm, m, s: [tm.cancel(0), tm.cancel(1), tm.cancel(2), tm.cancel(3), tm.cancel(4), B.same])


def test_tag_ff_is_reserved():
    bad = typed.MessageType("Bad", 0xFF)
    with pytest.raises(typed.CompileError):
        lower(lambda tm, m, s: [tm.start_single_timer("k", bad(1), 1), B.same])
    with pytest.raises(typed.CompileError):
        lower(lambda tm, m, s: [tm.cancel("k"), typed.self_ref(1).tell(bad(0)), B.same])
    with pytest.raises(typed.CompileError):
        lower(lambda tm, m, s: [tm.cancel("k"), B.same], test=lambda m: m.tag == 0xFF)
    # without timers the tag is an ordinary one
    b = typed.ReceiveBuilder.create(ST).on_message(bad, lambda m, s: [typed.self_ref(1).tell(bad(0)), B.same]).build("p")
    typed.compile_behaviors([b])


def test_setup_start_needs_constants():
    def build(timers):
        timers.start_single_timer("k", typed.Incoming.arg, 1)
        return typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same]).build("t")
    with pytest.raises(typed.CompileError):
        B.with_timers(build)
