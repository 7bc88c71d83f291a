"""Supervision on the GPU (agx_set_supervision; TY/internal/Supervision.scala:43-52,128-160,311-406): the HIP engine
through the C ABI against the known answers restated from the reference's SupervisionSpec
(tests/golden/supervision_kats.json) and against the model of DESIGN.md §2.5 (tests/supervision_model.py, itself
pinned to the frozen oracle by tests/test_supervision_model.py), on the fused and the multi-pass pipelines, with
graph replays and eager launches.  Everything is compared bit for bit after every run: states, alive flags,
kinds, every counter, the outbox order, supervision_info and read_supervision of every actor."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import supervision_cases as sc
from tests.supervision_model import SupervisionModel

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = 1, 5, 6
B = typed.Behaviors
S = typed.SupervisorStrategy


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the timers' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


@pytest.fixture(params=["replays", "eager"])
def launch(request, monkeypatch):
    if request.param == "eager":
        monkeypatch.setenv("AGX_NO_GRAPH", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = SupervisionModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def status_of(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def both(w, script, actors=None):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run; returns the last stats and snapshot, the outbox that of all runs"""
    eng, mod = engine_for(w), model_for(w)
    actors = range(w.n_actors) if actors is None else actors
    n = 0
    sent = []
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = sc.counts(sg), sc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = sc.snapshot(eng, actors), sc.snapshot(mod, actors)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert np.array_equal(eng.read_kinds(), mod.kind.astype(np.uint8))
        assert conserved(sg) and g["info"]["ticks"] == sg["supersteps"]
        sent += list(zip(*m["outbox"]))
        n += 1
    eng.close()
    m["outbox"] = sorted(sent, key=lambda x: x[0])   # (stable: every sender's envelopes in emission order)
    return sm, m


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(sc.kat_workload(name, T))
    got = sc.run_kat(name, T, eng)
    eng.close()
    print(got)
    sc.check_kat(name, T, got)
    assert got == sc.run_kat(name, T, model_for(sc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. shapes: buckets, windows, become
@pytest.mark.parametrize("n", [96, 70])
def test_shapes(built, pipeline, launch, n):
    """three buckets of 32 (the last one partial at 70): failures in the first and the last actor of a bucket, two
    failures of one actor inside one drain window, a failure as the last message before a `stopped`, a restart
    after a become (the kind returns to the initial one), an uncaught class, the limit exceeded"""
    st, snap = both(sc.mix_workload(n, 3), sc.shapes_script(n))
    assert snap["info"]["restarts"] >= 10 and snap["info"]["stops"] >= 4
    assert [snap["alive"][a] for a in (0, 5, 6, 7, 8)] == [0, 0, 0, 0, 0] and snap["alive"][n - 1] == 1


# ------------------------------------------------------------------ 3. the limit passes outwards; inner counts cleared
def test_limit_passes_to_the_outer_resume(built, pipeline, launch):
    sup = (("E1", [1, 50]), ("E1", "resume"), ("E3", "restart"))
    E1, E3 = 0, 2

    def script(t):
        sc.tells(t, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, E1), (33, sc.MIX_THROW, E1))
        yield t.run()    # the inner entry restarts
        sc.tells(t, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, E1), (3, sc.MIX_ECHO, 0))
        yield t.run()    # its limit of 1 is reached and time is left: the outer resume
        sc.tells(t, (3, sc.MIX_THROW, E3))
        yield t.run()    # the outer restart clears the inner counts
        sc.tells(t, (3, sc.MIX_THROW, E1))
        yield t.run()    # ... so the inner entry restarts again
    st, snap = both(sc.mix_workload(64, 1, sup), script)
    assert snap["info"] == dict(failures=5, resumes=1, restarts=4, stops=0, ticks=st["supersteps"])
    assert snap["sup"][3][1] == [1, 0, 1, 0]


# ------------------------------------------------------------------ 4. a window that spans two runs
def test_time_does_not_pass_between_runs(built, pipeline, launch):
    """limit 2 within 3 ticks, throughput 1: failures at ticks 1, 2 (the limit), two Incs, failures at ticks 5, 6 in a
    new window -- with run(1) steps and with one run()"""
    msgs = [(3, sc.MIX_THROW, 0)] * 2 + [(3, sc.MIX_INC, 0)] * 2 + [(3, sc.MIX_THROW, 0)] * 2

    def stepped(t):
        sc.tells(t, *msgs)
        for _ in range(6):
            yield t.run(1)
        yield t.run()

    def at_once(t):
        sc.tells(t, *msgs)
        yield t.run()
    a, b = both(sc.mix_workload(64, 1), stepped), both(sc.mix_workload(64, 1), at_once)
    assert a == b and a[1]["info"]["restarts"] == 4 and a[1]["alive"][3] == 1 and a[1]["sup"][3][1][0] == 2


# ------------------------------------------------------------------ 5. a bounded mailbox
def test_failure_that_stops_in_a_bounded_mailbox(built, pipeline):
    def script(t):
        sc.tells(t, (3, sc.MIX_INC, 1), (3, sc.MIX_THROW, 2), *[(3, sc.MIX_INC, 2)] * 4, (40, sc.MIX_THROW, 0))
        yield t.run(1)
        yield t.run()
    st, snap = both(sc.mix_workload(64, 2, capacity=4), script)
    assert st["dead_letters"] == 4 and snap["alive"][3] == 0 and snap["alive"][40] == 1


# ------------------------------------------------------------------ 6. the limits, each with its status
def plain_engine(**cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1), **cfg)))
    eng.register_range(0, 64, Kind.COUNTER)
    return eng


ROWS = [[typed.AgxSupervisor(class_mask=1, strategy=typed.SUP_RESTART, max_restarts=-1, within=1)]]


def test_refuses_bad_tables(built):
    eng = plain_engine()
    bad = lambda **kw: [[typed.AgxSupervisor(**dict(dict(class_mask=1, strategy=typed.SUP_RESTART, max_restarts=-1, within=1), **kw))]]
    for rows in (bad(strategy=0), bad(strategy=4), bad(within=0), bad(max_restarts=-2), bad(reset_mask=4), [ROWS[0] * 5], []):
        assert status_of(lambda: eng.set_supervision(rows)) == EINVAL
    eng.set_supervision(ROWS)
    eng.close()


def test_refuses_max_emit(built):
    eng = plain_engine(max_emit=2)
    assert status_of(lambda: eng.set_supervision(ROWS)) == EINVAL
    eng.close()


def test_refuses_the_other_features_either_order(built):
    table = bytes(range(256))
    for first in ("supervision", "other"):
        for other in ("priority", "stash", "timers", "watch"):
            eng = plain_engine()
            eng.set_mailbox_class(1, 0)
            set_other = {"priority": lambda: eng.set_mailbox_priority(1, table), "stash": lambda: eng.set_stash(1, 4),
                         "timers": lambda: eng.set_timers(1), "watch": lambda: eng.set_death_watch(1)}[other]
            if first == "supervision":
                eng.set_supervision(ROWS)
                with pytest.raises(AgxError) as e:
                    set_other()
            else:
                set_other()
                with pytest.raises(AgxError) as e:
                    eng.set_supervision(ROWS)
            eng.close()
            assert e.value.status == EINVAL and "supervision" in str(e.value)


def test_refuses_crdt_either_order(built):
    eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1))
    eng.set_supervision(ROWS)
    assert status_of(lambda: eng.register_range(0, 64, Kind.GCOUNTER)) == EINVAL
    eng.close()
    eng = engine_for(wl.crdt_gossip(64, Kind.GCOUNTER, rounds=1))
    assert status_of(lambda: eng.set_supervision(ROWS)) == EINVAL
    eng.close()


def test_refuses_after_the_first_run(built):
    eng = plain_engine()
    eng.tell(0, 1)
    eng.run()
    assert status_of(lambda: eng.set_supervision(ROWS)) == ESTATE
    eng.close()


def test_refuses_more_than_one_rank(built):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    with pytest.raises(AgxError) as e:
        eng.set_supervision(ROWS)
    eng.close()
    assert e.value.status == EINVAL and "n_ranks" in str(e.value)


def test_refused_on_a_ring_pool(built, monkeypatch):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    monkeypatch.setenv("AGX_NO_FUSED", "1")
    monkeypatch.setenv("AGX_RING_APPLY", "1")
    from tests.prio_cases import echo_population
    eng = engine_for(echo_population(3, 8))   # bounded FIFO actors: the per-actor rings come up at the first run
    eng.tell(np.arange(8, dtype=np.uint32), 1 << 24)
    eng.run()
    with pytest.raises(AgxError) as e:
        eng.set_supervision(ROWS)
    eng.close()
    assert e.value.status == EINVAL and "rings" in str(e.value) and "supervision" in str(e.value)


def test_failing_tables_without_supervision(built):
    """tables with AGX_RES_FAIL, or with a PreRestart / PostStop case alone, on an engine without supervision:
    agx_run returns AGX_EINVAL"""
    w = sc.mix_workload(64, 3)
    w.supervision = {}
    eng = engine_for(w)
    eng.tell(3, sc.MIX_INC << 24)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    b = (typed.ReceiveBuilder.create(typed.State("n", "unused")).on_any_message(lambda m, s: [s.n.inc(), B.same])
         .on_signal(typed.PostStop, lambda sig, s: [B.same]).build("signal_only"))
    tb = typed.compile_behaviors([b], max_emit=1)
    eng = engine_for(wl.Workload("signal_only", 64, 2, 1, 3, 0, [(0, 64, tb.kind_of(b), None)], behaviors=tb))
    eng.tell(3, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


def test_other_features_tables_on_a_supervision_engine(built):
    """tables with watch, timer or stash content on an engine with supervision: agx_run returns AGX_EINVAL"""
    from tests import watch_cases
    st = typed.State("n", "unused")
    timed = B.with_timers(lambda tm: typed.ReceiveBuilder.create(st).on_any_message(
        lambda m, s: [tm.start_single_timer("k", 1, 2), B.same]).build("timed"))
    stashing = B.with_stash(4, lambda buf: typed.ReceiveBuilder.create(st).on_any_message(
        lambda m, s: [s.n.inc(), buf.stash(), B.same]).build("stashing"))
    for b in (watch_cases.mix_behavior(64), timed, stashing):
        tb = typed.compile_behaviors([b], max_emit=1)
        eng = engine_for(wl.Workload("other", 64, 2, 1, 3, 0, [(0, 64, tb.kind_of(b), None)], behaviors=tb,
                                     supervision={"rows": ROWS}))
        eng.tell(3, 1 << 24)
        with pytest.raises(AgxError) as e:
            eng.run()
        eng.close()
        assert e.value.status == EINVAL and "supervision" in str(e.value)


def test_refuses_too_many_tells_and_bad_signal_cases(built):
    """hand-made tables (typed.py refuses them earlier): a failing case that tells beside a PreRestart case that
    tells is AGX_EINVAL at agx_run; a PreRestart case that does not end in same is AGX_EINVAL at agx_set_behaviors"""
    def tables(signal_result):
        A = typed
        tell = A.AgxAct(op=A.A_TELL, src=A.V_CONST, k=1, dsrc=A.V_CONST, dk=0)
        cases = [A.AgxCase(cmp1=A.CMP_ANY, cmp2=A.CMP_ANY, result=A.RES_FAIL, next=0, act_first=0, act_count=1),
                 A.AgxCase(src1=A.V_PAYLOAD, cmp1=A.CMP_EQ, src2=A.V_CONST, k2=A.SIGNAL_PRERESTART, cmp2=A.CMP_ANY,
                           result=A.CASE_SIGNAL | signal_result, act_first=1, act_count=1)]
        return A.Tables([A.Behavior("b", A.State())], (A.AgxCase * 2)(*cases), (A.AgxAct * 2)(tell, tell),
                        np.asarray([0, 2], np.uint32), 2)
    eng = plain_engine()
    eng.register_range(0, 64, typed.KIND_COMPILED)
    eng.set_supervision(ROWS)
    assert status_of(lambda: eng.set_behaviors(tables(typed.RES_STOPPED))) == EINVAL
    eng.set_behaviors(tables(typed.RES_SAME))
    eng.tell(3, 1)
    with pytest.raises(AgxError) as e:
        eng.run()
    eng.close()
    assert e.value.status == EINVAL and "max_emit" in str(e.value)


def test_over_one_tile(built, pipeline):
    """the skew launches know no supervision: 2049 tells to one bucket of 32 actors is AGX_ECAPACITY with its own
    message, sticky, and the engine closes cleanly"""
    eng = engine_for(sc.mix_workload(64, 3))
    eng.tell(np.full(2049, 41, np.uint32), np.full(2049, sc.MIX_INC << 24, np.uint32), np.full(2049, NO_SENDER, np.uint32))
    with pytest.raises(AgxError) as e:
        eng.run(1)
    assert e.value.status == ECAPACITY and "supervision" in str(e.value)
    assert status_of(lambda: eng.run(1)) == ECAPACITY   # (sticky)
    eng.close()


# ------------------------------------------------------------------ 7. the workload
def test_flaky_workers(built, pipeline, launch):
    w = wl.flaky_workers(4096, bucket_actors=32)

    def script(t):
        yield t.run(2)
        yield t.run()
    st, snap = both(w, script, actors=range(0, 4096, 7))
    assert snap["info"]["stops"] > 0 and snap["info"]["restarts"] > 100 and st["in_flight"] == 0
