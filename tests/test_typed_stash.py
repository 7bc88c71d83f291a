"""The stash in the compiled-behaviour DSL (akka_amd/typed.py): how with_stash / stash / unstash_all /
buffer.size lower into agx_case, that the case stays 48 bytes, and what the lowering refuses."""
import ctypes

import pytest

from akka_amd import typed
from akka_amd.typed import Behaviors, CompileError, ReceiveBuilder, State


def _gate(capacity=7):
    st = State("count")

    def build(buf):
        closed, opened = typed.Behavior("closed", st), typed.Behavior("open", st)
        (ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [buf.unstash_all(opened)], test=lambda m: m.tag == 1)
         .on_any_message(lambda m, s: [buf.unstash_all(Behaviors.same)], test=lambda m: m.tag == 2)
         .on_any_message(lambda m, s: [Behaviors.unhandled], when=lambda m, s: buf.is_full)
         .on_any_message(lambda m, s: [s.count.inc(), buf.stash(), Behaviors.same])
         .build(into=closed))
        (ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [typed.actor_ref(99).tell(buf.size), Behaviors.same], when=lambda m, s: buf.is_empty)
         .on_any_message(lambda m, s: [closed])
         .build(into=opened))
        return closed
    return Behaviors.with_stash(capacity, build)


def test_case_layout_unchanged():
    assert ctypes.sizeof(typed.AgxCase) == 48 and ctypes.sizeof(typed.AgxAct) == 32
    assert (typed.RES_SAME, typed.RES_STOPPED, typed.RES_UNHANDLED, typed.RES_BECOME) == (0, 1, 2, 3)
    assert (typed.RES_STASH, typed.RES_UNSTASH_ALL, typed.NEXT_SAME, typed.V_STASH) == (4, 5, 0xFF, 7)


def test_lowering():
    tb = typed.compile_behaviors([_gate()], max_emit=1)
    assert tb.n_behaviors == 2 and tb.stash_capacity == 7 and tb.max_tells == 1
    c = tb.cases
    assert (c[0].result, c[0].next) == (typed.RES_UNSTASH_ALL, 1)            # unstash_all(open): the reachable target
    assert (c[1].result, c[1].next) == (typed.RES_UNSTASH_ALL, typed.NEXT_SAME)
    assert (c[2].src1, c[2].cmp1, c[2].src2, c[2].k2) == (typed.V_STASH, typed.CMP_GE, typed.V_CONST, 7)  # is_full
    assert (c[3].result, c[3].act_count) == (typed.RES_STASH, 1)             # the stash effect is the result
    assert tb.acts[c[3].act_first].op == typed.A_ADD
    assert (c[4].src1, c[4].cmp1, c[4].k2) == (typed.V_STASH, typed.CMP_EQ, 0)                            # is_empty
    assert tb.acts[c[4].act_first].src == typed.V_STASH                      # buffer.size as a value
    assert (c[5].result, c[5].next) == (typed.RES_BECOME, 0)


def test_no_stash_no_capacity():
    assert typed.compile_behaviors([typed.echo(5)]).stash_capacity == 0


@pytest.mark.parametrize("result", [Behaviors.stopped, Behaviors.unhandled])
def test_stash_with_stopped_or_unhandled(result):
    with pytest.raises(CompileError):
        Behaviors.with_stash(3, lambda buf: ReceiveBuilder.create(State()).on_any_message(
            lambda m, s: [buf.stash(), result]).build())


def test_stash_with_unstash_all_or_become():
    other = typed.echo(5)
    for res in (lambda buf: buf.unstash_all(Behaviors.same), lambda buf: other):
        with pytest.raises(CompileError):
            Behaviors.with_stash(3, lambda buf: ReceiveBuilder.create(State()).on_any_message(
                lambda m, s: [buf.stash(), res(buf)]).build())


def test_stash_must_be_last_effect_and_bounded():
    with pytest.raises(CompileError):
        Behaviors.with_stash(3, lambda buf: ReceiveBuilder.create(State("n")).on_any_message(
            lambda m, s: [buf.stash(), s.n.inc(), Behaviors.same]).build())
    for cap in (0, 256, -1):
        with pytest.raises(CompileError):
            Behaviors.with_stash(cap, lambda buf: typed.echo(5))
