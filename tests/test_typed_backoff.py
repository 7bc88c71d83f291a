"""SupervisorStrategy.restart_with_backoff in akka_amd.typed: the lowering to the backoff rows (include/akka_gpu.h
agx_backoff) beside the supervisor entries, Tables.uses_backoff, and every CompileError.  No GPU."""
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.typed import (Behaviors as B, CompileError, ExceptionType, PreRestart, ReceiveBuilder, State,
                            SupervisorStrategy as S)


def worker(st, *excs):
    host = typed.actor_ref(99)
    rb = ReceiveBuilder.create(st)
    for i, e in enumerate(excs):
        rb.on_any_message(lambda m, s, e=e: [B.throw(e)], test=lambda m, i=i: m.tag == i + 1)
    rb.on_any_message(lambda m, s: [s.n.inc(), B.same])
    rb.on_signal(PreRestart, lambda sig, s: [host.tell(2), B.same])
    return rb.build("worker")


def row(r):
    return (r.min_backoff, r.max_backoff, r.random_factor_q16, r.reset_after, r.stash_capacity)


def test_lowering():
    st = State("n", "k")
    e1, e2 = ExceptionType("E1"), ExceptionType("E2")
    b = worker(st, e1, e2)
    bo = S.restart_with_backoff(3, 48, 0.2).with_max_restarts(5).with_reset_backoff_after(9).with_stash_capacity(2)
    b = B.supervise(b, reset={st.n: 5}).on_failure(bo, exc=e1)
    b = B.supervise(b).on_failure(S.restart.with_limit(2, 9), exc=e2)
    b = B.supervise(b).on_failure(S.resume)
    tb = typed.compile_behaviors([b], max_emit=1)
    assert tb.uses_supervision and tb.uses_backoff
    inner, mid, outer = tb.supervisors[0]
    assert (inner.strategy, inner.max_restarts, inner.reset_mask, inner.reset[0]) == (typed.SUP_RESTART, 5, 1, 5)
    assert (mid.strategy, mid.max_restarts, mid.within) == (typed.SUP_RESTART, 2, 9) and outer.strategy == typed.SUP_RESUME
    assert [row(r) for r in tb.backoff[0]] == [(3, 48, 13107, 9, 2), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]
    assert [len(r) for r in tb.backoff] == [len(r) for r in tb.supervisors]


def test_defaults_are_the_references():
    s = S.restart_with_backoff(4, 40, 0.0)
    assert (s.kind, s.max_restarts, s.reset_after, s.stash_capacity, s.random_factor_q16) == (typed.SUP_RESTART, -1, 4, -1, 0)
    assert S.restart_with_backoff(1, 1, 1.0).random_factor_q16 == 65536
    assert s.with_stash_capacity(0).stash_capacity == 0 and s.stash_capacity == -1   # (a value: the chain copies)
    assert not hasattr(s, "with_limit")


def test_plain_tables_use_no_backoff():
    st = State("n", "k")
    b = B.supervise(worker(st, ExceptionType("E"))).on_failure(S.restart)
    tb = typed.compile_behaviors([b], max_emit=1)
    assert tb.uses_supervision and not tb.uses_backoff and [row(r) for r in tb.backoff[0]] == [(0, 0, 0, 0, 0)]
    assert not typed.compile_behaviors([typed.library()["counter"]]).uses_backoff
    assert not wl.flaky_workers(64).behaviors.uses_backoff and "backoff" not in wl.flaky_workers(64).supervision


@pytest.mark.parametrize("args", [(0, 4, 0.0), (5, 4, 0.0), (1, 1 << 31, 0.0), (1.5, 4, 0.0), (1, 4, -0.1), (1, 4, 1.5),
                                  (1, 4, "x"), (True, 4, 0.0)])
def test_bad_arguments(args):
    with pytest.raises(CompileError):
        S.restart_with_backoff(*args)


@pytest.mark.parametrize("call", [lambda s: s.with_max_restarts(-2), lambda s: s.with_max_restarts(1.5),
                                  lambda s: s.with_reset_backoff_after(0), lambda s: s.with_reset_backoff_after(1 << 31),
                                  lambda s: s.with_stash_capacity(-2), lambda s: s.with_stash_capacity("3")])
def test_bad_chained_arguments(call):
    with pytest.raises(CompileError):
        call(S.restart_with_backoff(1, 4, 0.0))


def supervised(extra=None):
    st = State("n", "k")
    rb = ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [B.throw(typed.Throwable)], test=lambda m: m.tag == 1)
    if extra is not None:
        extra(rb, st)
    rb.on_any_message(lambda m, s: [s.n.inc(), B.same])
    return B.supervise(rb.build("w")).on_failure(S.restart_with_backoff(1, 4, 0.0))


def test_backoff_with_what_supervision_refuses():
    with pytest.raises(CompileError, match="max_emit = 1"):
        typed.compile_behaviors([supervised()], max_emit=2)

    st = State("n", "k")
    bo = S.restart_with_backoff(1, 4, 0.0)
    watching = (ReceiveBuilder.create(st).on_any_message(lambda m, s: [typed.context.watch(typed.actor_ref(1)), B.same])
                .build("watching"))
    timed = B.with_timers(lambda tm: ReceiveBuilder.create(st).on_any_message(
        lambda m, s: [tm.start_single_timer("k", 1, 2), B.same]).build("timed"))
    stashing = B.with_stash(4, lambda buf: ReceiveBuilder.create(st)
                            .on_any_message(lambda m, s: [buf.stash(), B.same], test=lambda m: m.tag == 1)
                            .on_any_message(lambda m, s: [B.same]).build("stashing"))
    for b in (watching, timed, stashing):
        with pytest.raises(CompileError, match="restart_with_backoff lives on the supervision engine"):
            typed.compile_behaviors([B.supervise(b).on_failure(bo)])
    a = typed.Behavior("a", st)
    b = B.supervise(ReceiveBuilder.create(st).on_any_message(lambda m, s: [a]).build("b")).on_failure(bo)
    ReceiveBuilder.create(st).on_any_message(lambda m, s: [b]).build(into=a)
    with pytest.raises(CompileError, match="reached by become"):
        typed.compile_behaviors([b, a], max_emit=1)
    with pytest.raises(CompileError, match="at most"):
        x = supervised()
        for _ in range(typed.MAX_SUPERVISORS):
            x = B.supervise(x).on_failure(bo)


def test_the_workloads_lower_to_rows():
    for w in (wl.backoff_workers(256), wl.backoff_stash_pressure(256)):
        tb = w.behaviors
        assert tb.uses_backoff and w.supervision["backoff"] is tb.backoff and w.supervision["rows"] is tb.supervisors
    assert [r[0].stash_capacity for r in wl.backoff_stash_pressure(256).behaviors.backoff[1:]] == [0, 1, 2, -1]
