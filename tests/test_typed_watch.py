"""The death watch surface of the compiled-behaviour DSL (akka_amd.typed: context.watch / watch_with / unwatch,
ReceiveBuilder.on_signal, Behaviors.receive_signal), without a GPU: the lowering and every CompileError."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.typed import CompileError

B = typed.Behaviors
ctx = typed.context
ST = typed.State("a", "b")


def lower(*behaviors):
    return typed.compile_behaviors(list(behaviors), max_emit=1)


def test_action_encodings():
    """the ref is the d-operand, where a TELL has its destination; watchWith's message is the operand, as a TELL's
    payload"""
    down = typed.MessageType("Down", 7)
    b = (typed.ReceiveBuilder.create(ST)
         .on_any_message(lambda m, s: [ctx.watch(m.sender), ctx.watch_with(typed.self_ref(1), down(s.a)),
                                       ctx.watch_with(typed.actor_ref(9), m.payload + 1), ctx.unwatch(s.b.ref), B.same])
         .build("w"))
    tb = lower(b)
    acts = [tb.acts[i] for i in range(tb.n_acts)]
    assert [a.op for a in acts] == [typed.A_WATCH, typed.A_WATCH_WITH, typed.A_WATCH_WITH, typed.A_UNWATCH] == [10, 11, 11, 12]
    assert (acts[0].dsrc, acts[0].dword, acts[0].dk, acts[0].or_mask) == (typed.V_SENDER, 0, 0, 0)
    assert (acts[1].dsrc, acts[1].dk, acts[1].src, acts[1].sword, acts[1].or_mask) == (typed.V_SELF, 1, typed.V_WORD, 0, 7 << 24)
    assert (acts[2].dsrc, acts[2].dk, acts[2].src, acts[2].k, acts[2].or_mask) == (typed.V_CONST, 9, typed.V_PAYLOAD, 1, 0)
    assert (acts[3].dsrc, acts[3].dword) == (typed.V_WORD, 1)
    assert tb.uses_watch and tb.timer_keys == 0 and tb.max_tells == 0
    assert tb.cases[0].result == typed.RES_SAME  # (an ordinary case: no signal flag)


def test_signal_flag_and_receive_signal():
    nxt = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same]).build("next")
    b = (typed.ReceiveBuilder.create(ST)
         .on_any_message(lambda m, s: [B.same])
         .on_signal(typed.Terminated, lambda sig, s: [s.a.set(sig.ref.dst), sig.ref.tell(1), B.stopped],
                    when=lambda sig, s: sig.ref.dst == 5)
         .on_signal(typed.Terminated, lambda sig, s: [nxt])
         .build("b"))
    B.receive_signal(b, lambda sig, s: [B.unhandled])
    tb = lower(b)
    res = [tb.cases[i].result for i in range(int(tb.first[1]))]
    S = typed.CASE_SIGNAL
    assert S == 0x80 and res == [typed.RES_SAME, S | typed.RES_STOPPED, S | typed.RES_BECOME, S | typed.RES_UNHANDLED]
    c = tb.cases[1]  # the guard reads the terminated ref as the sender
    assert (c.src1, c.cmp1, c.src2, c.k2) == (typed.V_SENDER, typed.CMP_EQ, typed.V_CONST, 5)
    assert tb.cases[2].next == 1 and tb.uses_watch
    assert typed.SIGNAL_TERMINATED == 0xFE000001 and typed.TAG_WATCH == 0xFE


def test_uses_watch():
    plain = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [s.a.inc(), B.same]).build("plain")
    assert not lower(plain).uses_watch
    only_unwatch = typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [ctx.unwatch(m.sender), B.same]).build("u")
    assert lower(only_unwatch).uses_watch
    only_signal = (typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same])
                   .on_signal(typed.Terminated, lambda sig, s: [B.same]).build("s"))
    assert lower(only_signal).uses_watch
    assert lower(wl.watch_ring(8).behaviors.behaviors[0]).uses_watch
    assert not wl.death_pact_chain(8).behaviors.uses_watch  # (the chain is set up from the host and handles nothing)


def test_tag_fe_is_reserved():
    for make in (lambda m, s: [ctx.watch(m.sender), typed.self_ref(1).tell(1, tag=0xFE), B.same],
                 lambda m, s: [ctx.watch_with(m.sender, typed.MessageType("X", 0xFE)(0)), B.same]):
        with pytest.raises(CompileError, match="0xFE"):
            lower(typed.ReceiveBuilder.create(ST).on_any_message(make).build("b"))
    with pytest.raises(CompileError, match="0xFE"):
        lower(typed.ReceiveBuilder.create(ST)
              .on_message(typed.MessageType("X", 0xFE), lambda m, s: [ctx.watch(m.sender), B.same]).build("b"))
    # without death watch the tag is an ordinary one
    lower(typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [typed.self_ref(1).tell(1, tag=0xFE), B.same]).build("b"))


def test_signal_case_errors():
    rb = typed.ReceiveBuilder.create(ST)
    with pytest.raises(CompileError, match="Terminated"):
        rb.on_signal(object, lambda sig, s: [B.same])

    def stashing(buf):
        return (typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same])
                .on_signal(typed.Terminated, lambda sig, s: [buf.stash(), B.same]).build("b"))
    with pytest.raises(CompileError, match="stash"):
        B.with_stash(4, stashing)

    def unstashing(buf):
        return (typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same])
                .on_signal(typed.Terminated, lambda sig, s: [buf.unstash_all(B.same)]).build("b"))
    with pytest.raises(CompileError, match="stash"):
        B.with_stash(4, unstashing)

    def timing(timers):
        return (typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same])
                .on_signal(typed.Terminated, lambda sig, s: [timers.start_single_timer("k", 1, 1), B.same]).build("b"))
    with pytest.raises(CompileError, match="timers"):
        B.with_timers(timing)

    def testing(timers):
        return (typed.ReceiveBuilder.create(ST).on_any_message(lambda m, s: [B.same])
                .on_signal(typed.Terminated, lambda sig, s: [B.same], when=lambda sig, s: timers.is_timer_active("k")).build("b"))
    with pytest.raises(CompileError, match="timers"):
        B.with_timers(testing)


def test_watch_and_timers_do_not_share_tables():
    def build(timers):
        return (typed.ReceiveBuilder.create(ST)
                .on_any_message(lambda m, s: [timers.cancel("k"), ctx.watch(m.sender), B.same]).build("b"))
    with pytest.raises(CompileError, match="timers"):
        lower(B.with_timers(build))


def test_not_a_ref():
    for call in (lambda: ctx.watch(5), lambda: ctx.unwatch(ST.a), lambda: ctx.watch_with(typed.Operand(typed.V_SENDER), 1)):
        with pytest.raises(CompileError, match="ActorRef"):
            call()
