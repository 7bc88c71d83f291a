"""Behaviors.supervise / Behaviors.throw / PreRestart / PostStop in akka_amd.typed: the lowering to the case tables
and the supervisor entries (include/akka_gpu.h agx_supervisor), the exception hierarchy as masks, and every
CompileError.  No GPU."""
import pytest

from akka_amd import typed
from akka_amd.typed import (Behaviors as B, CompileError, ExceptionType, PostStop, PreRestart, ReceiveBuilder, State,
                            SupervisorStrategy as S, Throwable)


def worker(st, *excs, pre_tells=0, fail_tells=0):
    host = typed.actor_ref(99)
    rb = ReceiveBuilder.create(st)
    for i, e in enumerate(excs):
        rb.on_any_message(lambda m, s, e=e: [host.tell(1)] * fail_tells + [B.throw(e)], test=lambda m, i=i: m.tag == i + 1)
    rb.on_any_message(lambda m, s: [s.n.inc(), B.same])
    rb.on_signal(PreRestart, lambda sig, s: [host.tell(2)] * pre_tells + [s.k.set(7), B.same])
    return rb.build("worker")


def test_lowering():
    st = State("n", "k")
    e1 = ExceptionType("E1")
    e2 = ExceptionType("E2", e1)
    e3 = ExceptionType("E3")
    b = worker(st, e2, e3, pre_tells=1)
    b = B.supervise(b, reset={st.n: 5}).on_failure(S.restart.with_limit(2, 9), exc=e1)
    b = B.supervise(b).on_failure(S.resume, exc=e3)
    b = B.supervise(b, reset={"k": 1}).on_failure(S.stop)
    tb = typed.compile_behaviors([b], max_emit=1)
    assert tb.uses_supervision and not tb.uses_watch and tb.timer_keys == 0
    assert tb.exception_classes == [e2, e3, e1]   # thrown classes first, then the supervisors'
    c = tb.cases
    assert (c[0].result, c[0].next) == (typed.RES_FAIL, 0) and (c[1].result, c[1].next) == (typed.RES_FAIL, 1)
    sig = c[3]
    assert sig.result == typed.CASE_SIGNAL | typed.RES_SAME
    assert (sig.src1, sig.k1, sig.cmp1, sig.src2, sig.k2) == (typed.V_PAYLOAD, 0, typed.CMP_EQ, typed.V_CONST, typed.SIGNAL_PRERESTART)
    rows = tb.supervisors
    assert len(rows) == 1 and len(rows[0]) == 3
    inner, mid, outer = rows[0]
    assert (inner.class_mask, inner.strategy, inner.max_restarts, inner.within) == (0b101, typed.SUP_RESTART, 2, 9)
    assert (inner.reset_mask, inner.reset[0]) == (1, 5)
    assert (mid.class_mask, mid.strategy, mid.reset_mask) == (0b010, typed.SUP_RESUME, 0)
    assert (outer.class_mask, outer.strategy, outer.reset_mask) == (0xFFFFFFFF, typed.SUP_STOP, 0)   # (reset: restarts only)
    assert S.restart.max_restarts == -1 and S.restart.kind == typed.SUP_RESTART


def test_unsupervised_throw_and_poststop_alone_use_supervision():
    st = State("n", "k")
    tb = typed.compile_behaviors([worker(st, ExceptionType("E"))], max_emit=1)
    assert tb.uses_supervision and tb.supervisors == [[]]
    b = ReceiveBuilder.create(st).on_any_message(lambda m, s: [B.same]).build("quiet")
    b = B.receive_signal(b, lambda sig, s: [s.n.inc(), B.same], signal=PostStop)
    tb = typed.compile_behaviors([b])
    assert tb.uses_supervision and not tb.uses_watch and tb.cases[1].k2 == typed.SIGNAL_POSTSTOP
    plain = typed.compile_behaviors([typed.library()["counter"]])
    assert not plain.uses_supervision and plain.supervisors == [[]]


def test_the_root_catches_all_and_parents_catch_children():
    root_child = ExceptionType("A")
    assert root_child.parent is Throwable and root_child.is_a(Throwable) and not Throwable.is_a(root_child)
    st = State("n", "k")
    a, b_, c = ExceptionType("A"), ExceptionType("B"), None
    c = ExceptionType("C", b_)
    beh = B.supervise(worker(st, a, b_, c)).on_failure(S.restart, exc=b_)
    row = typed.compile_behaviors([beh], max_emit=1).supervisors[0]
    assert row[0].class_mask == 0b110


@pytest.mark.parametrize("make", [
    lambda st: B.throw("boom"),
    lambda st: ExceptionType("E", parent="Exception"),
    lambda st: B.supervise("not a behavior"),
    lambda st: B.supervise(worker(st, ExceptionType("E"))).on_failure("restart"),
    lambda st: B.supervise(worker(st, ExceptionType("E"))).on_failure(S.restart, exc="E"),
    lambda st: B.supervise(worker(st, ExceptionType("E")), reset={"nope": 1}),
    lambda st: B.supervise(worker(st, ExceptionType("E")), reset={st.n: -1}),
    lambda st: S.restart.with_limit(-1, 5),
    lambda st: S.restart.with_limit(2, 0),
    lambda st: S.restart.with_limit(2, 1.5),
    lambda st: ReceiveBuilder.create(st).on_signal(PreRestart, lambda sig, s: [B.stopped]),
    lambda st: ReceiveBuilder.create(st).on_signal(PostStop, lambda sig, s: [worker(st)]),
    lambda st: ReceiveBuilder.create(st).on_signal(PostStop, lambda sig, s: [typed.context.watch(typed.actor_ref(1)), B.same]),
    lambda st: ReceiveBuilder.create(st).on_signal(object, lambda sig, s: [B.same]),
])
def test_compile_errors_at_the_call(make):
    with pytest.raises(CompileError):
        make(State("n", "k"))


def test_more_than_four_supervisors():
    st = State("n", "k")
    b = worker(st, ExceptionType("E"))
    for _ in range(4):
        b = B.supervise(b).on_failure(S.resume)
    with pytest.raises(CompileError):
        B.supervise(b).on_failure(S.resume)


def test_more_than_32_classes():
    st = State("n", "k")
    rb = ReceiveBuilder.create(st)
    for i in range(33):
        rb.on_any_message(lambda m, s, e=ExceptionType(f"E{i}"): [B.throw(e)], test=lambda m, i=i: m.arg == i)
    with pytest.raises(CompileError):
        typed.compile_behaviors([rb.build("many")])


def test_tells_of_a_failing_case_and_a_signal_case():
    st = State("n", "k")
    e = ExceptionType("E")
    typed.compile_behaviors([worker(st, e, pre_tells=1)], max_emit=1)
    typed.compile_behaviors([worker(st, e, fail_tells=1)], max_emit=1)
    with pytest.raises(CompileError):
        typed.compile_behaviors([worker(st, e, pre_tells=1, fail_tells=1)], max_emit=1)
    stopping = (ReceiveBuilder.create(st).on_any_message(lambda m, s: [typed.actor_ref(9).tell(1), B.stopped])
                .on_signal(PostStop, lambda sig, s: [typed.actor_ref(9).tell(2), B.same]).build("stopping"))
    with pytest.raises(CompileError):
        typed.compile_behaviors([stopping])


def test_max_emit_stays_1():
    with pytest.raises(CompileError):
        typed.compile_behaviors([worker(State("n", "k"), ExceptionType("E"))], max_emit=2)


def test_supervise_around_a_behaviour_reached_by_become():
    st = State("n", "k")
    inner = B.supervise(worker(st, ExceptionType("E"))).on_failure(S.restart)
    outer = ReceiveBuilder.create(st).on_any_message(lambda m, s: [inner]).build("outer")
    with pytest.raises(CompileError):
        typed.compile_behaviors([outer])


def test_supervision_shares_tables_with_no_other_feature():
    st = State("n", "k")
    e = ExceptionType("E")
    watching = (ReceiveBuilder.create(st).on_any_message(lambda m, s: [typed.context.watch(typed.actor_ref(1)), B.throw(e)])
                .build("watching"))
    timed = B.with_timers(lambda tm: ReceiveBuilder.create(st).on_any_message(
        lambda m, s: [tm.start_single_timer("k", 1, 2), B.throw(e)]).build("timed"))
    stashing = B.with_stash(4, lambda buf: ReceiveBuilder.create(st)
                            .on_any_message(lambda m, s: [buf.stash(), B.same], test=lambda m: m.tag == 1)
                            .on_any_message(lambda m, s: [B.throw(e)]).build("stashing"))
    terminated = (ReceiveBuilder.create(st).on_any_message(lambda m, s: [B.throw(e)])
                  .on_signal(typed.Terminated, lambda sig, s: [B.same]).build("terminated"))
    for b in (watching, timed, stashing, terminated):
        with pytest.raises(CompileError):
            typed.compile_behaviors([b])
