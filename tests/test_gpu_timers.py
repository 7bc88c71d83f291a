"""Timers on the GPU (agx_set_timers; TimerSchedulerImpl.scala:61-172): the HIP engine through the C ABI
against the known answers restated from the reference's TimerSpec (tests/golden/timer_kats.json), against the
model of DESIGN.md §2.3 (tests/timer_model.py, itself pinned to the frozen oracle by
tests/test_timer_model.py) and -- where no timer is in use -- against the frozen FIFO oracle, on the fused and
the multi-pass pipelines.  The observable for order is an echo to a host id (the outbox keeps each sender's
order)."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import timer_cases as tc
from tests.prio_model import per_sender
from tests.test_prio_model import same
from tests.test_timer_model import run_oracle
from tests.timer_model import TimerModel

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ECAPACITY, ESTATE = 1, 2, 5, 6
SLOT_KEYS = ("active", "remaining", "period", "payload", "generation")
B = typed.Behaviors


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the stash's fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = TimerModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def conserved(st, info):
    return st["staged"] + st["emitted"] + info["fired"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def echo_workload(n, T, bucket_actors, n_keys=2, capacity=0, host_n=1):
    """actors that echo every message's payload to the host id n (a TimerMsg: the slot's stored payload)"""
    st = typed.State("count", "unused")
    host = typed.actor_ref(n)

    def build(timers):
        for k in range(n_keys):
            timers.cancel(k)  # (the keys 0..n_keys-1, in order)
        return (typed.ReceiveBuilder.create(st)
                .on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same]).build("echo"))
    b = B.with_timers(build)
    tb = typed.compile_behaviors([b], max_emit=1)
    return wl.Workload("timer_echo", n, 2, 1, T, capacity, [(0, n, tb.kind_of(b), None)], behaviors=tb,
                       outbound=(n, host_n), bucket_actors=bucket_actors, timers={"n_keys": n_keys})


def status_of(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", tc.KAT_T)
@pytest.mark.parametrize("name", tc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(tc.kat_workload(name, T))
    got = tc.run_kat(name, T, eng)
    eng.close()
    print(got)
    tc.check_kat(name, T, got)
    assert got == tc.run_kat(name, T, model_for(tc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. a bucket whose only work is a fire
def test_fire_only_bucket(built, pipeline):
    """2 buckets of 128 actors, one single timer of delay 7 in the second, no mail at all"""
    w = echo_workload(256, 3, 128)
    eng = engine_for(w)
    eng.start_timers(200, 1, 0, 7, payload=0x01000042)
    ticks, echoes, again = [], [], []
    for budget in (3, 3, None):
        st = eng.run() if budget is None else eng.run(budget)
        ticks.append(eng.timer_info()["ticks"])
        echoes.append(eng.take_outbound()[2].tolist())
        again.append(eng.pump_idle())  # (a pending timer keeps the pump scheduled)
    info = eng.timer_info()
    eng.close()
    assert ticks == [3, 6, 7] and echoes == [[], [], [0x01000042]] and again == [True, True, False]
    assert info == dict(fired=1, discarded=0, active=0, pending=0, ticks=7)
    assert st.supersteps == 1 and st.delivered == 1 and st.in_flight == 0  # (only tick 7 had mail)


# ------------------------------------------------------------------ 3. the inbox order of a tick
def test_inbox_order(built, pipeline):
    """an arrival, a staged tell and two keys due in one tick: arrival, staged, key 0, key 1"""
    # the arrival: actor 8 forwards to actor 9 (a behaviour of its own)
    st = typed.State("count", "unused")
    host = typed.actor_ref(64)

    made = {}

    def build(timers):
        timers.cancel(0), timers.cancel(1)  # (the keys 0 and 1)
        made["echo"] = (typed.ReceiveBuilder.create(st)
                        .on_any_message(lambda m, s: [s.count.inc(), host.tell(m.payload), B.same]).build("echo"))
        return (typed.ReceiveBuilder.create(st)
                .on_any_message(lambda m, s: [typed.self_ref(1).tell(m.payload), B.same]).build("fwd"))
    fwd = B.with_timers(build)
    echo = made["echo"]
    tb = typed.compile_behaviors([fwd, echo], max_emit=1)
    w = wl.Workload("timer_order", 64, 2, 1, 5, 0, [(0, 64, tb.kind_of(echo), None), (8, 1, tb.kind_of(fwd), None)],
                    behaviors=tb, outbound=(64, 1), bucket_actors=32, timers={"n_keys": 2})
    got = []
    for target in (engine_for(w), model_for(w)):
        target.start_timers(9, 1, 1, 2, payload=0x01000001)  # key 1 first: the order is by key, not by start
        target.start_timers(9, 1, 0, 2, payload=0x01000000)
        target.tell(8, 0x03000003)          # tick 1: actor 8 forwards it: an arrival for actor 9 at tick 2
        target.run(1)
        target.tell(9, 0x04000004)          # staged for tick 2
        target.run(1)
        got.append(target.take_outbound()[2].tolist())
        target.close()
    assert got[0] == [0x03000003, 0x04000004, 0x01000000, 0x01000001] and got[1] == got[0]


# ------------------------------------------------------------------ 4. periods against replay boundaries
@pytest.mark.parametrize("launch", ["replays", "replays_of_2", "eager"])
@pytest.mark.parametrize("budgets", [(40,), (33,), (3, 16, 21)])
def test_periods(built, pipeline, budgets, launch, monkeypatch):
    """periods 1, 5, 16 and 17: the fire counts are the model's whatever the replay sizes -- graph replays of up
    to 16 supersteps, of at most 2, and eager supersteps"""
    if launch == "eager":
        monkeypatch.setenv("AGX_NO_GRAPH", "1")
    elif launch == "replays_of_2":
        monkeypatch.setenv("AGX_MAX_REPLAY", "2")
    w = echo_workload(160, 3, 32, n_keys=1)
    got = []
    for target in (engine_for(w), model_for(w)):
        for i, period in enumerate((1, 5, 16, 17)):
            target.start_timers(40 * i + 3, 2, 0, period, periodic=True, payload=period)
        for b in budgets:
            st = target.run(b)
        words, _ = target.read_state()
        got.append((words[:, 0].tolist(), target.timer_info(), sorted(target.take_outbound()[2].tolist())))
        target.close()
    assert got[0] == got[1]
    n = sum(budgets)
    assert got[0][1]["fired"] == 2 * (n + n // 5 + n // 16 + n // 17) and got[0][1]["ticks"] == n


# ------------------------------------------------------------------ 5. a full bounded mailbox
def test_bounded_full_at_the_fire(built, pipeline):
    """capacity 2, full at the fire: the TimerMsg is a dead letter, `fired` counts it, the single slot stays
    active with nothing to come, and the engine goes quiescent"""
    w = echo_workload(64, 1, 32, n_keys=1, capacity=2)
    got = []
    for target in (engine_for(w), model_for(w)):
        target.start_timers(5, 1, 0, 2, payload=0x01000007)
        p = np.asarray([0x02000001, 0x02000002, 0x02000003], np.uint32)
        target.tell(np.full(3, 5, np.uint32), p, np.full(3, NO_SENDER, np.uint32))  # tick 1: 2 admitted, 1 drained
        target.run(1)
        target.tell(5, 0x02000004)  # tick 2: backlog 1 + staged 1 = full; the TimerMsg is third
        st = tc.counts(target.run())
        info = target.timer_info()
        slot = target.read_timers(5)
        got.append((st, info, {k: int(slot[k][0]) for k in SLOT_KEYS}, target.take_outbound()[2].tolist()))
        target.close()
    assert got[0] == got[1]
    st, info, slot, echo = got[0]
    assert info["fired"] == 1 and info["active"] == 1 and info["pending"] == 0 and info["discarded"] == 0
    assert slot["active"] == 1 and slot["remaining"] == 0xFFFFFFFF and st["dead_letters"] == 2 and st["in_flight"] == 0
    assert echo == [0x02000001, 0x02000002, 0x02000004] and conserved(st, info)


# ------------------------------------------------------------------ 6. starts from the host between runs
def test_start_between_runs(built, pipeline):
    w = echo_workload(300, 3, 128, n_keys=2)
    got = []
    for target in (engine_for(w), model_for(w)):
        target.start_timers(0, 300, 0, 4, payload=0x01000000)
        target.run(2)
        target.start_timers(100, 150, 1, 3, periodic=True, delays=1 + np.arange(150) % 5, payload=0x02000000)
        target.start_timers(10, 5, 0, 1, payload=0x03000000)  # (replaces key 0: the next generation)
        st = tc.counts(target.run(9))
        o = per_sender(*target.take_outbound())
        slots = [{k: target.read_timers(a)[k].tolist() for k in SLOT_KEYS} for a in (0, 12, 100, 249, 250)]
        got.append((st, target.timer_info(), o.tolist(), slots))
        target.close()
    assert got[0] == got[1]
    assert got[0][1]["ticks"] == 11 and got[0][3][1]["generation"][0] == 2 and conserved(got[0][0], got[0][1])


# ------------------------------------------------------------------ 7. population parity
@pytest.mark.parametrize("bucket_actors", [128, 2048])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("seed", [1, 2])
def test_population(built, pipeline, seed, T, bucket_actors):
    n = 2048 + 37  # (a last bucket that is not full)
    w = wl.heartbeat(n, 7, seed=seed, throughput=T, bucket_actors=bucket_actors)
    eng, mod = engine_for(w), model_for(w)
    for budget in (3, 40):
        sg, sm = tc.counts(eng.run(budget)), tc.counts(mod.run(budget))
        ig, im = eng.timer_info(), mod.timer_info()
        assert same((sg, eng.read_state(), eng.take_outbound()), (sm, mod.read_state(), mod.take_outbound())) is None
        assert ig == im and conserved(sg, ig)
        assert np.array_equal(eng.read_kinds(), mod.kind.astype(np.uint8))
    for a in range(n):
        g, m = eng.read_timers(a), mod.read_timers(a)
        assert all(np.array_equal(g[k], m[k]) for k in SLOT_KEYS), (a, g, m)
    eng.close()
    assert ig["ticks"] == 43 and ig["discarded"] > 0 and ig["fired"] > n


# ------------------------------------------------------------------ 8. timers set, none started: the frozen oracle
def test_unused_timers_equal_the_oracle(built, pipeline):
    w = wl.priority_mix(2048, tables=False)
    w.timers = {"n_keys": 4}
    eng = engine_for(w)
    st = tc.counts(eng.run())
    got = (st, eng.read_state(), eng.take_outbound())
    info = eng.timer_info()
    eng.close()
    assert same(got, run_oracle(w)) is None
    assert {k: info[k] for k in tc.INFO_KEYS} == dict(fired=0, discarded=0, active=0, pending=0)


# ------------------------------------------------------------------ 9. the limits, each with its status
def plain_engine(**cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1), **cfg)))
    eng.register_range(0, 64, Kind.COUNTER)
    return eng


@pytest.mark.parametrize("n_keys", [0, 5])
def test_refuses_bad_key_count(built, n_keys):
    eng = plain_engine()
    assert status_of(lambda: eng.set_timers(n_keys)) == EINVAL
    eng.close()


def test_refuses_max_emit(built):
    eng = plain_engine(max_emit=2)
    assert status_of(lambda: eng.set_timers(1)) == EINVAL
    eng.close()


def test_refuses_priority_and_stash_either_order(built):
    table = bytes(range(256))
    for first in ("timers", "other"):
        for other in ("priority", "stash"):
            eng = plain_engine()
            eng.set_mailbox_class(1, 0)
            set_other = (lambda: eng.set_mailbox_priority(1, table)) if other == "priority" else (lambda: eng.set_stash(1, 4))
            if first == "timers":
                eng.set_timers(2)
                assert status_of(set_other) == EINVAL
            else:
                set_other()
                assert status_of(lambda: eng.set_timers(2)) == EINVAL
            eng.close()


def test_refuses_crdt_either_order(built):
    eng = GpuEngine(EngineConfig(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1))
    eng.set_timers(1)
    assert status_of(lambda: eng.register_range(0, 64, Kind.GCOUNTER)) == EINVAL
    eng.close()
    w = wl.crdt_gossip(64, Kind.GCOUNTER, rounds=1)
    eng = engine_for(w)
    assert status_of(lambda: eng.set_timers(1)) == EINVAL
    eng.close()


def test_refuses_after_the_first_run(built):
    eng = plain_engine()
    eng.tell(0, 1)
    eng.run()
    assert status_of(lambda: eng.set_timers(1)) == ESTATE
    eng.close()


def test_refuses_tag_ff_tells(built):
    """agx_stage_tells (eng.tell) and agx_tell (eng.tell_one) both refuse the TimerMsg tag"""
    eng = plain_engine()
    eng.set_timers(1)
    assert status_of(lambda: eng.tell(0, 0xFF000001)) == EINVAL
    assert status_of(lambda: eng.tell_one(0, 0xFF000001)) == EINVAL
    eng.tell(0, 0xFE000001)
    eng.tell_one(0, 0xFE000002)
    st = eng.run()
    eng.close()
    assert st.delivered == 2 and st.staged == 2
    eng = plain_engine()  # without timers the tag is an ordinary one
    eng.tell(0, 0xFF000001)
    eng.tell_one(0, 0xFF000002)
    assert eng.run().delivered == 2
    eng.close()


def test_refuses_more_than_one_rank(built):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    with pytest.raises(AgxError) as e:
        eng.set_timers(1)
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
        eng.set_timers(1)
    eng.close()
    # (agx_set_timers looks at the ring pool before it looks at `started`: this message means the pool exists)
    assert e.value.status == EINVAL and "rings" in str(e.value) and "timers" in str(e.value)


def active_test_workload(key_names, tested):
    """actors that count a message only while timer `tested` is active: tables whose only use of timers is
    AGX_V_TIMER (is_timer_active); `key_names` are mapped to the slots 0.. in order"""
    st = typed.State("count", "unused")

    def build(timers):
        for k in key_names:
            timers.cancel(k)
        return (typed.ReceiveBuilder.create(st)
                .on_any_message(lambda m, s: [s.count.inc(), B.same], when=lambda m, s: timers.is_timer_active(tested))
                .on_any_message(lambda m, s: [B.same])
                .build("counts_while_active"))
    b = B.with_timers(build)
    tb = typed.compile_behaviors([b], max_emit=1)
    assert not any(tb.acts[i].op >= typed.A_TIMER_SINGLE for i in range(tb.n_acts))  # (no timer action in the tables)
    return wl.Workload("timer_active", 64, 2, 1, 3, 0, [(0, 64, tb.kind_of(b), None)], behaviors=tb, bucket_actors=32)


def test_timer_tables_without_timers(built):
    """tables with a timer action, tables with AGX_V_TIMER alone, or start_timers, on an engine without timers:
    agx_run returns AGX_EINVAL"""
    w = tc.kat_workload("repeated", 5)   # (a timer action)
    w.timers = {}
    eng = engine_for(w)
    eng.tell(tc.ACTOR, tc.payload("Bump"))
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    eng = engine_for(active_test_workload(["a"], "a"))   # (is_timer_active alone)
    eng.tell(3, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    eng = plain_engine()
    assert status_of(lambda: eng.start_timers(0, 1, 0, 1)) == EINVAL
    eng.tell(0, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


def test_start_refused_before_set_timers_does_not_stick(built):
    """a start refused for want of timers no longer stands in the way once timers are set"""
    w = echo_workload(64, 3, 32, n_keys=1)
    w.timers = {}
    eng = engine_for(w)
    assert status_of(lambda: eng.start_timers(5, 1, 0, 2, payload=7)) == EINVAL
    eng.set_timers(1)
    eng.start_timers(5, 1, 0, 2, payload=7)
    st = eng.run()
    info = eng.timer_info()
    eng.close()
    assert st.delivered == 1 and info == dict(fired=1, discarded=0, active=0, pending=0, ticks=2)


def test_keys_past_n_keys(built):
    """a key >= n_keys: agx_start_timers refuses it, and tables that use one make agx_run return AGX_EINVAL"""
    eng = plain_engine()
    eng.set_timers(1)
    assert status_of(lambda: eng.start_timers(0, 1, 1, 1)) == EINVAL
    eng.close()
    w = active_test_workload(["a", "b"], "b")   # is_timer_active of key 1 ...
    w.timers = {"n_keys": 1}                    # ... on an engine with one key
    eng = engine_for(w)
    eng.tell(3, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()
    w.timers = {"n_keys": 2}                    # with two keys the same tables run: the slot is inactive, no count
    eng = engine_for(w)
    eng.start_timers(4, 1, 1, 9)
    eng.tell(np.asarray([3, 4], np.uint32), 1)
    st = eng.run(1)
    words, _ = eng.read_state()
    eng.close()
    assert st.delivered == 2 and words[3, 0] == 0 and words[4, 0] == 1
    def build(timers):                          # a timer action of key 1 ...
        timers.cancel("x")
        return (typed.ReceiveBuilder.create(typed.State("count", "unused"))
                .on_any_message(lambda m, s: [timers.start_single_timer("y", 1, 1), B.same]).build("starts_key_1"))
    b = B.with_timers(build)
    tb = typed.compile_behaviors([b], max_emit=1)
    w = wl.Workload("timer_key1", 64, 2, 1, 3, 0, [(0, 64, tb.kind_of(b), None)], behaviors=tb, bucket_actors=32,
                    timers={"n_keys": 1})   # ... on an engine with one key
    eng = engine_for(w)
    eng.tell(3, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


# AGX_ENOMEM (the slots do not fit) has no test: it can only be provoked by exhausting the memory of a GPU that
# other processes share -- agx_create itself allocates the population's state first, so an engine large enough
# for the slots to fail takes nearly all of it -- and an allocation failure on such a device is not a state a
# test suite should drive it into.  The path is the hipMalloc check of alloc_timers (agx_engine.hip).


def test_over_one_tile(built, pipeline):
    """the skew launches know no timers: a bucket over one 2048-message tile is AGX_ECAPACITY, sticky"""
    w = echo_workload(64, 3, 32, n_keys=1)
    eng = engine_for(w)
    eng.start_timers(40, 1, 0, 1, periodic=True, payload=5)   # due at tick 1, in the bucket that overflows
    eng.start_timers(41, 1, 0, 1, payload=6)
    eng.tell(np.full(2049, 40, np.uint32), np.arange(2049, dtype=np.uint32), np.full(2049, NO_SENDER, np.uint32))
    assert status_of(lambda: eng.run(1)) == ECAPACITY
    # the state stays defined: the bucket's mail was dropped, and the slots due in that tick moved on as if they
    # had fired (a periodic one a period on, a single one with none to come) -- none is left overdue
    per, single = eng.read_timers(40), eng.read_timers(41)
    assert per["active"][0] == 1 and per["remaining"][0] == 1 and per["period"][0] == 1
    assert single["active"][0] == 1 and single["remaining"][0] == 0xFFFFFFFF
    assert eng.timer_info()["pending"] == 1
    assert status_of(lambda: eng.run(1)) == ECAPACITY   # (sticky)
    eng.close()
