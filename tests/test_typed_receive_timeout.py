"""typed.context.set_receive_timeout / cancel_receive_timeout and compile_behaviors(transparent=...): the lowering
to AGX_A_SET_RECEIVE_TIMEOUT / AGX_A_CANCEL_RECEIVE_TIMEOUT and every CompileError (no GPU)."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import receive_timeout_cases as rc

B = typed.Behaviors
ctx = typed.context
TIMEOUT, TT = typed.MessageType("Timeout", 2), typed.MessageType("TransparentTick", 4)


def idle_behavior(effects, state=None, name="idle"):
    st = state or typed.State("count", "unused")
    return typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: list(effects(m, s)) + [B.same]).build(name)


def test_lowering():
    b = idle_behavior(lambda m, s: [ctx.set_receive_timeout(m.arg + 1, TIMEOUT(s.count)), ctx.cancel_receive_timeout(),
                                    ctx.set_receive_timeout(7, 0x0300002A)])
    tb = typed.compile_behaviors([b], max_emit=1, transparent=(TT, typed.MessageType("Identify", 5), TT))
    a = [tb.acts[i] for i in range(tb.n_acts)]
    assert [x.op for x in a] == [typed.A_SET_RECEIVE_TIMEOUT, typed.A_CANCEL_RECEIVE_TIMEOUT, typed.A_SET_RECEIVE_TIMEOUT] == [15, 16, 15]
    # the delay in the d-operand (where a TELL has its destination), the message as a TELL's payload
    assert (a[0].dsrc, a[0].dk, a[0].src, a[0].sword, a[0].or_mask) == (typed.V_ARG, 1, typed.V_WORD, 0, 2 << 24)
    assert (a[2].dsrc, a[2].dk, a[2].src, a[2].k, a[2].or_mask) == (typed.V_CONST, 7, typed.V_CONST, 0x0300002A, 0)
    assert tb.uses_receive_timeout and tb.transparent_tags == (4, 5)
    assert tb.timer_keys == 0 and tb.max_tells == 0 and not tb.uses_watch and not tb.uses_children


def test_tables_without_a_receive_timeout():
    tb = typed.compile_behaviors([typed.library()["counter"]], transparent=(TT,))
    assert not tb.uses_receive_timeout and tb.transparent_tags == (4,)
    assert typed.compile_behaviors([typed.library()["counter"]]).transparent_tags == ()


def test_only_a_receive_timeout_still_needs_a_timer_key():
    """Tables.timer_keys is 0 for such behaviours; the workloads pass n_keys = max(timer_keys, 1) to set_timers"""
    w = rc.become_workload(3, 4)
    assert w.behaviors.timer_keys == 0 and w.timers["n_keys"] == 1 and "receive_timeout" in w.timers
    p = wl.passivating_entities(96, 3, idle=3)
    # (the entities' timeout comes from the setup block alone: no action of the tables sets or cancels one)
    assert not p.behaviors.uses_receive_timeout and p.behaviors.timer_keys == 0 and p.timers["n_keys"] == 1
    assert p.timers["receive_timeout"]["starts"] == [(0, 96, 3, wl.PE_IDLE << 24)] and p.max_emit == 1


@pytest.mark.parametrize("delay", [0, -3, 1 << 31])
def test_constant_delay_out_of_range(delay):
    with pytest.raises(typed.CompileError, match="a receive timeout is at (least 1 tick|most)"):
        ctx.set_receive_timeout(delay, TIMEOUT())


def test_transparent_takes_message_types():
    with pytest.raises(typed.CompileError, match="transparent= takes MessageTypes"):
        typed.compile_behaviors([typed.library()["counter"]], transparent=(4,))


def test_max_emit_above_one():
    b = idle_behavior(lambda m, s: [ctx.cancel_receive_timeout()])
    with pytest.raises(typed.CompileError, match="receive timeouts need max_emit = 1, not 2"):
        typed.compile_behaviors([b], max_emit=2)
    typed.compile_behaviors([b])  # (no max_emit given: the engine checks)


@pytest.mark.parametrize("where", ["message_type", "test", "tell_tag", "transparent"])
def test_tag_fb_is_reserved(where):
    odd = typed.MessageType("Odd", 0xFB)
    st = typed.State("count", "unused")
    rb = typed.ReceiveBuilder.create(st)
    transparent = ()
    if where == "message_type":
        rb.on_message(odd, lambda m, s: [ctx.set_receive_timeout(3, TIMEOUT()), B.same])
    elif where == "test":
        rb.on_any_message(lambda m, s: [ctx.cancel_receive_timeout(), B.same], test=lambda m: m.tag != 0xFB)
    elif where == "tell_tag":
        rb.on_any_message(lambda m, s: [ctx.cancel_receive_timeout(), typed.self_ref(1).tell(odd(1)), B.same])
    else:
        rb.on_any_message(lambda m, s: [ctx.cancel_receive_timeout(), B.same])
        transparent = (odd,)
    with pytest.raises(typed.CompileError, match="message tag 0xFB is reserved for the receive-timeout envelope"):
        typed.compile_behaviors([rb.build("fb")], max_emit=1, transparent=transparent)


def test_the_timeout_message_itself_may_not_carry_fb():
    b = idle_behavior(lambda m, s: [ctx.set_receive_timeout(3, typed.MessageType("Odd", 0xFB)())])
    with pytest.raises(typed.CompileError, match="message tag 0xFB is reserved"):
        typed.compile_behaviors([b], max_emit=1)


def test_tag_ff_is_reserved_too():
    """an engine with receive timeouts has timers: the TimerMsg's tag stays reserved though no timer is used"""
    b = idle_behavior(lambda m, s: [ctx.set_receive_timeout(3, typed.MessageType("Odd", 0xFF)())])
    with pytest.raises(typed.CompileError, match="message tag 0xFF is reserved for timer messages"):
        typed.compile_behaviors([b], max_emit=1)


def test_tag_fb_without_a_receive_timeout_is_an_ordinary_tag():
    b = (typed.ReceiveBuilder.create(typed.State("count", "unused"))
         .on_message(typed.MessageType("Odd", 0xFB), lambda m, s: [s.count.inc(), B.same]).build("fb"))
    assert not typed.compile_behaviors([b], max_emit=1).uses_receive_timeout


TOGETHER = "receive timeouts live on the timer engine, which shares an engine with neither a stash, death watch, children nor supervision"


def test_not_with_a_stash():
    def build(buffer):
        return (typed.ReceiveBuilder.create(typed.State("count", "unused"))
                .on_message(TT, lambda m, s: [buffer.stash(), B.same])
                .on_any_message(lambda m, s: [ctx.set_receive_timeout(3, TIMEOUT()), B.same]).build("stashes"))
    with pytest.raises(typed.CompileError, match=TOGETHER):
        typed.compile_behaviors([B.with_stash(4, build)], max_emit=1)


def test_not_with_death_watch():
    b = idle_behavior(lambda m, s: [ctx.watch(typed.self_ref(1)), ctx.set_receive_timeout(3, TIMEOUT())])
    with pytest.raises(typed.CompileError, match=TOGETHER):
        typed.compile_behaviors([b], max_emit=1)
    sig = (typed.ReceiveBuilder.create(typed.State("count", "unused"))
           .on_signal(typed.Terminated, lambda sig, s: [ctx.cancel_receive_timeout(), B.same])
           .on_any_message(lambda m, s: [B.same]).build("signal_case"))
    with pytest.raises(typed.CompileError, match=TOGETHER):
        typed.compile_behaviors([sig], max_emit=1)


def test_not_with_children():
    child = idle_behavior(lambda m, s: [], name="child")
    b = idle_behavior(lambda m, s: [ctx.spawn(child), ctx.set_receive_timeout(3, TIMEOUT())], name="parent")
    with pytest.raises(typed.CompileError, match=TOGETHER):
        typed.compile_behaviors([b], max_emit=1)


def test_not_with_supervision():
    b = idle_behavior(lambda m, s: [ctx.set_receive_timeout(3, TIMEOUT())])
    sup = B.supervise(b).on_failure(typed.SupervisorStrategy.resume)
    with pytest.raises(typed.CompileError, match="supervision shares an engine with neither|" + TOGETHER):
        typed.compile_behaviors([sup], max_emit=1)
    with pytest.raises(typed.CompileError):   # a PreRestart case that touches the timeout is refused where it is built
        (typed.ReceiveBuilder.create(typed.State("count", "unused"))
         .on_signal(typed.PreRestart, lambda sig, s: [ctx.cancel_receive_timeout(), B.same]))


def test_with_timers_is_fine():
    for name in rc.KAT_NAMES:
        tb = rc.kat_workload(name, 5).behaviors
        assert tb.uses_receive_timeout and tb.timer_keys == 3 and tb.transparent_tags == (4, 5)
