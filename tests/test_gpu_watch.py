"""Death watch on the GPU (agx_set_death_watch; AA/dungeon/DeathWatch.scala:19-113): the HIP engine through the C
ABI against the known answers restated from the reference's WatchSpec (tests/golden/watch_kats.json), against the
model of DESIGN.md §2.4 (tests/watch_model.py, itself pinned to the frozen oracle by tests/test_watch_model.py)
and -- where no watch is in use -- against the frozen FIFO oracle, on the fused and the multi-pass pipelines.
Everything is compared bit for bit: states, alive flags, kinds, every counter, the outbox order, watch_info
and read_watch."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import watch_cases as wc
from tests.test_prio_model import same
from tests.test_watch_model import run_oracle
from tests.watch_model import WatchModel

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ECAPACITY, ESTATE = 1, 2, 5, 6
B = typed.Behaviors


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
    m = WatchModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def status_of(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status


def conserved(st, info):
    return st["staged"] + st["emitted"] + info["terminated"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def both(w, script, actors=None):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run"""
    eng, mod = engine_for(w), model_for(w)
    actors = range(w.n_actors) if actors is None else actors
    n = 0
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = wc.counts(sg), wc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = wc.snapshot(eng, actors), wc.snapshot(mod, actors)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert np.array_equal(eng.read_kinds(), mod.kind.astype(np.uint8))
        assert conserved(sg, g["info"])
        n += 1
    eng.close()
    return sm, m


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", wc.KAT_T)
@pytest.mark.parametrize("name", wc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(wc.kat_workload(name, T))
    got = wc.run_kat(name, T, eng)
    eng.close()
    print(got)
    wc.check_kat(name, T, got)
    assert got == wc.run_kat(name, T, model_for(wc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. shapes: buckets, dead and unknown watchees
def tells(target, *msgs):
    d = np.asarray([m[0] for m in msgs], np.uint32)
    p = np.asarray([(m[1] << 24) | m[2] for m in msgs], np.uint32)
    target.tell(d, p, np.full(d.size, NO_SENDER, np.uint32))


@pytest.mark.parametrize("n", [96, 70])
def test_shapes(built, pipeline, launch, n):
    """watcher and watchee in one bucket and across buckets (the last one partial at 70), a watch of an actor that
    is dead already, of an id outside the population and of an id that was never registered, and the latencies: a
    death at tick s answers at s + 2, a watch of a dead actor at s + 1"""
    w = wc.mix_workload(n, 3)
    w.ranges = w.ranges + [(9, 1, Kind.NONE, None)]  # actor 9: never registered

    def script(t):
        tells(t, (3, wc.MIX_WATCH, 4), (40, wc.MIX_WITH, 4), (n - 1, wc.MIX_WATCH, 4), (n - 2, wc.MIX_WATCH, n - 1),
              (5, wc.MIX_WATCH, 9), (6, wc.MIX_WITH, n + 3), (4, wc.MIX_STOP, 0))
        yield t.run(1)   # tick 1: the watches, and actor 4 stops
        yield t.run(1)   # tick 2: the watches of 9 and n + 3 are answered (s + 1)
        yield t.run(1)   # tick 3: the death of 4 (s + 2)
        tells(t, (7, wc.MIX_WATCH, 4), (n - 1, wc.MIX_STOP, 0))
        yield t.run()
    st, snap = both(w, script)
    assert snap["info"]["ticks"] == 6 and snap["info"]["terminated"] == 7 and snap["info"]["watching"] == 0


# ------------------------------------------------------------------ 3. 64 watchers of one watchee
def test_fan_in(built, pipeline):
    w = wc.mix_workload(96, 5)
    w.watch = {"n_slots": 2, "starts": [(32, 32, np.full(32, 3, np.uint32), 0, None),
                                         (64, 32, np.full(32, 3, np.uint32), 0, wc.MIX_DOWN << 24 | 3)]}

    def script(t):
        tells(t, (3, wc.MIX_STOP, 0))
        yield t.run()
    st, snap = both(w, script)
    assert snap["info"]["terminated"] == 64 and snap["info"]["ticks"] == 3 and len(snap["outbox"][0]) == 64


# ------------------------------------------------------------------ 4. the workloads
def test_death_pact_chain(built, pipeline, launch):
    w = wl.death_pact_chain(40, bucket_actors=32)

    def script(t):
        yield t.run(30)   # (a budget that ends inside the chain)
        yield t.run()
    st, snap = both(w, script)
    assert sum(snap["alive"]) == 0 and snap["info"]["death_pacts"] == 39 and snap["info"]["ticks"] == 79


@pytest.mark.parametrize("kill", [(5,), (5, 50), (5, 6), (30, 31, 32, 95, 0)])
def test_watch_ring(built, pipeline, kill):
    w = wl.watch_ring(96, kill, bucket_actors=32)

    def script(t):
        yield t.run()
    st, snap = both(w, script)
    assert sum(snap["alive"]) == 96 - len(kill) and snap["info"]["watching"] == 96 - len(kill)
    assert sum(x[1] for x in snap["words"]) == len(kill)  # every loss is counted once


# ------------------------------------------------------------------ 5. budgets between the death and the receipt
def test_budgets_and_the_empty_tick(built, pipeline, launch):
    """the death comes in the last tick that has mail: the empty tick after it must run; budgets that end between
    the death and the receipt, then more runs; ticks = min(budget, ticks until quiescence)"""
    w = wc.mix_workload(96, 3)
    w.watch = {"n_slots": 1, "starts": [(70, 1, [2], 0, None)]}
    ticks = []

    def script(t):
        tells(t, (2, wc.MIX_STOP, 0))
        for budget in (1, 1, 5, 1 << 30):
            st = t.run(budget)
            ticks.append(t.watch_info()["ticks"])
            yield st
    st, snap = both(w, script)
    assert ticks == [1, 1, 2, 2, 3, 3, 3, 3] and snap["info"]["terminated"] == 1 and st["supersteps"] == 2


# ------------------------------------------------------------------ 6. a start between runs
def test_start_between_runs(built, pipeline):
    w = wc.mix_workload(96, 3)

    def script(t):
        t.start_watch(0, 96, offset=1)
        tells(t, (10, wc.MIX_STOP, 0), (50, wc.MIX_STOP, 0))
        yield t.run(2)
        t.start_watch(20, 40, offset=30, message=(wc.MIX_DOWN << 24) | 1)  # (some watchees are dead by now: due at once)
        t.start_watch(0, 4, np.asarray([10, 200, 1, 2], np.uint32))
        yield t.run()
    st, snap = both(w, script)
    assert snap["info"]["conflicts"] == 0 and snap["info"]["terminated"] == 5


def test_start_conflict_stops_the_actor(built, pipeline):
    w = wc.mix_workload(64, 3)

    def script(t):
        t.start_watch(5, 2, offset=7)
        t.start_watch(5, 1, offset=7, message=9)   # watchWith after watch: IllegalStateException
        t.start_watch(6, 1, offset=7)              # idempotent
        t.start_watch(30, 1, [5])                  # (5 is dead by now: due at once)
        yield t.run()
    st, snap = both(w, script)
    assert snap["alive"][5] == 0 and snap["alive"][6] == 1 and snap["info"]["conflicts"] == 1
    assert snap["info"]["terminated"] == 1


# ------------------------------------------------------------------ 7. a random mix
@pytest.mark.parametrize("n,T", [(96, 1), (70, 5)])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_mix(built, pipeline, seed, n, T):
    w = wc.mix_workload(n, T)
    rounds = wc.mix_rounds(n, seed)

    def script(t):
        for i, (dst, pay) in enumerate(rounds):
            t.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
            yield t.run(2 if i % 2 else 1 << 30)
        yield t.run()
    st, snap = both(w, script)
    assert snap["info"]["terminated"] > 0 and snap["info"]["watches"] > 20


def test_bounded_full_at_the_notification(built, pipeline):
    """capacity 2, full when the Terminated arrives: it is a dead letter, `terminated` counts it, the slot stays
    notified"""
    w = wc.mix_workload(64, 1, capacity=2)
    w.watch = {"n_slots": 1, "starts": [(40, 1, [2], 0, None)]}

    def script(t):
        tells(t, (2, wc.MIX_STOP, 0), (40, 9, 1), (40, 9, 2))
        yield t.run(1)        # tick 1: actor 2 stops; one message drained, one queued
        tells(t, (40, 9, 3))
        yield t.run(1)        # tick 2: the slot becomes due; again one queued
        tells(t, (40, 9, 4))  # tick 3: backlog 1 + staged 1 = full; the Terminated is third
        yield t.run()
    st, snap = both(w, script)
    assert snap["info"]["terminated"] == 1 and snap["slots"][40]["state"][0] == 3 and st["dead_letters"] == 1


# ------------------------------------------------------------------ 8. death watch set, none used: the frozen oracle
def test_unused_watch_equals_the_oracle(built, pipeline):
    w = wl.priority_mix(2048, tables=False)
    w.watch = {"n_slots": 4}
    eng = engine_for(w)
    st = wc.counts(eng.run())
    got = (st, eng.read_state(), eng.take_outbound())
    info = eng.watch_info()
    eng.close()
    assert same(got, run_oracle(w)) is None
    assert {k: info[k] for k in wc.INFO_KEYS} == dict.fromkeys(wc.INFO_KEYS, 0)


# ------------------------------------------------------------------ 9. the limits, each with its status
def plain_engine(**cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1), **cfg)))
    eng.register_range(0, 64, Kind.COUNTER)
    return eng


@pytest.mark.parametrize("n_slots", [0, 5])
def test_refuses_bad_slot_count(built, n_slots):
    eng = plain_engine()
    assert status_of(lambda: eng.set_death_watch(n_slots)) == EINVAL
    eng.close()


def test_refuses_max_emit(built):
    eng = plain_engine(max_emit=2)
    assert status_of(lambda: eng.set_death_watch(1)) == EINVAL
    eng.close()


def test_refuses_priority_stash_and_timers_either_order(built):
    table = bytes(range(256))
    for first in ("watch", "other"):
        for other in ("priority", "stash", "timers"):
            eng = plain_engine()
            eng.set_mailbox_class(1, 0)
            set_other = {"priority": lambda: eng.set_mailbox_priority(1, table), "stash": lambda: eng.set_stash(1, 4),
                         "timers": lambda: eng.set_timers(1)}[other]
            if first == "watch":
                eng.set_death_watch(2)
                assert status_of(set_other) == EINVAL
            else:
                set_other()
                assert status_of(lambda: eng.set_death_watch(2)) == EINVAL
            eng.close()


def test_refuses_crdt_either_order(built):
    eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1))
    eng.set_death_watch(1)
    assert status_of(lambda: eng.register_range(0, 64, Kind.GCOUNTER)) == EINVAL
    eng.close()
    eng = engine_for(wl.crdt_gossip(64, Kind.GCOUNTER, rounds=1))
    assert status_of(lambda: eng.set_death_watch(1)) == EINVAL
    eng.close()


def test_refuses_after_the_first_run(built):
    eng = plain_engine()
    eng.tell(0, 1)
    eng.run()
    assert status_of(lambda: eng.set_death_watch(1)) == ESTATE
    eng.close()


def test_refuses_tag_fe_tells(built):
    """agx_stage_tells (eng.tell) and agx_tell (eng.tell_one) both refuse the Terminated tag"""
    eng = plain_engine()
    eng.set_death_watch(1)
    assert status_of(lambda: eng.tell(0, 0xFE000001)) == EINVAL
    assert status_of(lambda: eng.tell_one(0, 0xFE000001)) == EINVAL
    eng.tell(0, 0xFF000001)
    st = eng.run()
    eng.close()
    assert st.delivered == 1 and st.staged == 1
    eng = plain_engine()  # without death watch the tag is an ordinary one
    eng.tell(0, 0xFE000001)
    eng.tell_one(0, 0xFE000002)
    assert eng.run().delivered == 2
    eng.close()


def test_refuses_more_than_one_rank(built):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    with pytest.raises(AgxError) as e:
        eng.set_death_watch(1)
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
        eng.set_death_watch(1)
    eng.close()
    assert e.value.status == EINVAL and "rings" in str(e.value) and "death watch" in str(e.value)


def test_watch_tables_without_death_watch(built):
    """tables with a watch action, tables with a signal case alone, or start_watch, on an engine without death
    watch: agx_run returns AGX_EINVAL"""
    w = wc.mix_workload(64, 3)
    w.watch = {}
    eng = engine_for(w)
    eng.tell(3, 9 << 24)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    b = (typed.ReceiveBuilder.create(typed.State("n", "unused")).on_any_message(lambda m, s: [s.n.inc(), B.same])
         .on_signal(typed.Terminated, lambda sig, s: [B.same]).build("signal_only"))
    tb = typed.compile_behaviors([b], max_emit=1)
    eng = engine_for(wl.Workload("signal_only", 64, 2, 1, 3, 0, [(0, 64, tb.kind_of(b), None)], behaviors=tb))
    eng.tell(3, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    eng = plain_engine()
    assert status_of(lambda: eng.start_watch(0, 1, [1])) == EINVAL
    eng.tell(0, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


# AGX_ENOMEM (the slots do not fit) has no test: it cannot be provoked safely on a device that other processes
# share.  The path is the hipMalloc check of alloc_watch (agx_engine.hip).


def test_over_one_tile(built, pipeline):
    """the skew launches know no death watch: a bucket over one 2048-message tile is AGX_ECAPACITY, sticky, and
    the due slot of that bucket still becomes notified"""
    w = wc.mix_workload(64, 3)
    w.watch = {"n_slots": 1, "starts": [(40, 1, [200], 0, None)]}   # due at once, in the bucket that overflows
    eng = engine_for(w)
    eng.tell(np.full(2049, 41, np.uint32), np.arange(2049, dtype=np.uint32) | (9 << 24), np.full(2049, NO_SENDER, np.uint32))
    assert status_of(lambda: eng.run(1)) == ECAPACITY
    assert eng.read_watch(40)["state"][0] == 3 and eng.watch_info()["pending"] == 0
    assert status_of(lambda: eng.run(1)) == ECAPACITY   # (sticky)
    eng.close()


def test_slot_exhaustion(built, pipeline):
    """a third watch with two slots: AGX_ECAPACITY with its own message, sticky; the watch is not recorded"""
    w = wc.mix_workload(64, 5, n_slots=2)
    eng = engine_for(w)
    tells(eng, (3, wc.MIX_WATCH, 10), (3, wc.MIX_WATCH, 11), (3, wc.MIX_WATCH, 12))
    with pytest.raises(AgxError) as e:
        eng.run()
    assert e.value.status == ECAPACITY and "watch slots" in str(e.value)
    assert eng.read_watch(3)["watchee"][:2].tolist() == [10, 11] and eng.watch_info()["watches"] == 2
    assert status_of(lambda: eng.run(1)) == ECAPACITY   # (sticky)
    eng.close()
    eng = engine_for(w)   # the same from the host's setup block
    eng.start_watch(3, 1, [10])
    eng.start_watch(3, 1, [11])
    eng.start_watch(3, 1, [12])
    assert status_of(lambda: eng.run()) == ECAPACITY
    eng.close()
