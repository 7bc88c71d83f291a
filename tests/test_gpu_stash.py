"""Deque-based mailboxes and the stash on the GPU (agx_set_stash; StashBufferImpl.scala:61-79,131-218):
the HIP engine through the C ABI against the reference specs' known answers
(tests/golden/stash_kats.json), against the model of DESIGN.md §2.2 (tests/stash_model.py, itself
pinned to the frozen oracle by tests/test_stash_model.py) and -- where no stash is in use -- against
the frozen FIFO oracle, on the fused and the multi-pass pipelines.  The observable for order is an
echo to a host id (the outbox keeps each sender's order)."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind
from tests import stash_cases as sc
from tests.prio_model import per_sender
from tests.stash_model import StashModel
from tests.test_prio_model import same
from tests.test_stash_model import run_oracle

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = 1, 5, 6


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the priority mailboxes' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = StashModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def snapshot(t, n):
    """everything the population tests compare, of an engine or the model"""
    st = sc.counts(t.run())
    words, alive = t.read_state()
    stash = [tuple(x.tolist() if hasattr(x, "tolist") else x for x in t.read_stash(a)) for a in range(n)]
    return st, words, alive, per_sender(*t.take_outbound()), t.stash_info(), stash, t.read_kinds().tolist()


# ------------------------------------------------------------------ 1. the four known answers
@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(sc.kat_workload(name, T))
    got = sc.run_kat(name, T, eng)
    eng.close()
    print(got)
    sc.check_kat(name, got)
    assert got == sc.run_kat(name, T, model_for(sc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. a bucket with nothing but released messages
def test_pending_only_bucket(built, pipeline):
    eng = engine_for(sc.small_gates(T=1))
    args = [5, 6, 7, 8]
    eng.tell(*sc.gate_msgs(wl.GATE_DATA, args))
    eng.tell(*sc.gate_msgs(wl.GATE_OPEN, [0]))
    st = sc.counts(eng.run())
    echo = eng.take_outbound()
    info = eng.stash_info()
    eng.close()
    assert echo[2].tolist() == sc.gate_msgs(wl.GATE_DATA, args)[1].tolist() and (echo[1] == sc.LAST).all()
    assert info == dict(stashed=4, unstashed=4, overflows=0, held=0, pending=0)
    assert st["delivered"] == 5 and st["in_flight"] == 0 and conserved(st) and st["supersteps"] == 9


# ------------------------------------------------------------------ 3. held messages do not keep the run going
def test_held_only_quiescence(built, pipeline):
    eng = engine_for(sc.small_gates(T=1))
    args = [5, 6, 7, 8]
    eng.tell(*sc.gate_msgs(wl.GATE_DATA, args))
    st = sc.counts(eng.run())
    info = eng.stash_info()
    assert st["in_flight"] == 4 and info["held"] == 4 and info["pending"] == 0 and conserved(st) and st["delivered"] == 0
    assert eng.read_stash(sc.LAST)[1].tolist() == sc.gate_msgs(wl.GATE_DATA, args)[1].tolist()
    eng.tell(*sc.gate_msgs(wl.GATE_OPEN, [0]))
    st = sc.counts(eng.run())
    echo = eng.take_outbound()[2]
    info = eng.stash_info()
    eng.close()
    assert echo.tolist() == sc.gate_msgs(wl.GATE_DATA, args)[1].tolist()
    assert st["in_flight"] == 0 and info["held"] == 0 and st["delivered"] == 5 and conserved(st)


# ------------------------------------------------------------------ 4. population parity against the model
@pytest.mark.parametrize("bucket_actors", sc.POPULATION_BUCKETS)
@pytest.mark.parametrize("seed,T", sc.POPULATION)
def test_population_parity(built, pipeline, seed, T, bucket_actors):
    w = wl.stash_gate(2048, seed=seed, throughput=T)
    eng, m = engine_for(w, bucket_actors=bucket_actors), model_for(w)
    s3, m3 = sc.counts(eng.run(3)), sc.counts(m.run(3))
    print(s3, m3)
    assert s3 == m3 and conserved(s3) and s3["in_flight"] > 0
    got, exp = snapshot(eng, w.n_actors), snapshot(m, w.n_actors)
    eng.close()
    print(got[0], got[4])
    assert got[0] == exp[0] and conserved(got[0])
    assert got[4] == exp[4]
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[1], exp[1])
    assert got[3].shape == exp[3].shape and np.array_equal(got[3], exp[3])
    assert got[5] == exp[5]
    assert got[6] == exp[6] and len(set(got[6])) == 2   # the kinds after become / unstash_all(next): both gates occur


# ------------------------------------------------------------------ 5. a stash class that no behaviour uses
@pytest.mark.parametrize("T", [1, 5])
def test_unused_stash_equals_oracle(built, pipeline, T):
    w = wl.priority_mix(2048, seed=5 + T, throughput=T, tables=False)
    w.stash = {1: 6, 2: 3}
    eng = engine_for(w, bucket_actors=128)
    st = sc.counts(eng.run())
    got = (st, eng.read_state(), eng.take_outbound())
    info = eng.stash_info()
    eng.close()
    assert same(got, run_oracle(w)) is None
    assert info == dict(stashed=0, unstashed=0, overflows=0, held=0, pending=0)


# ------------------------------------------------------------------ 6. stop with a non-empty buffer and park
def test_stop_with_buffer_and_park(built, pipeline):
    w = sc.stop_workload(3)
    eng = engine_for(w)
    got = sc.stop_script(eng)
    eng.close()
    print(got)
    assert got == sc.stop_script(model_for(w))
    assert got["mid"]["pending"] == 5 and got["mid"]["held"] == 0           # four released, one parked
    st = got["counts"]
    assert st["dead_letters"] == 4 and st["delivered"] == 3 and conserved(st) and st["in_flight"] == 0
    assert got["echo"] == sc.payloads(["Msg:m1"]).tolist() and got["alive"] == 0
    assert got["info"]["held"] == 0 and got["info"]["pending"] == 0


# ------------------------------------------------------------------ 7. a bounded class with a stash
def test_bounded_class_with_stash(built, pipeline):
    w = sc.small_gates(T=2, classes={1: 4}, mailboxes=[(64, 37, 1)], stash={0: 4, 1: 3})

    def script(t):
        t.tell(*sc.gate_msgs(wl.GATE_DATA, [1, 2, 3]))            # three held: the buffer is full (S = 3)
        t.run()
        t.tell(*sc.gate_msgs(wl.GATE_OPEN, [0]))
        t.tell(*sc.gate_msgs(wl.GATE_DATA, [4, 5, 6, 7, 8]))      # C = 4: Open and three Data admitted, two dropped
        st = sc.counts(t.run())
        return st, t.stash_info(), t.take_outbound()[2].tolist(), t.read_stash(sc.LAST)[1].tolist()

    eng = engine_for(w)
    got = script(eng)
    eng.close()
    assert got == script(model_for(w))
    st, info, echo, _ = got
    assert st["dead_letters"] == 2 and len(echo) == 6 and conserved(st) and info["overflows"] == 0


# ------------------------------------------------------------------ 8. a stash case on a class without a stash
def test_stash_case_without_capacity_stops(built, pipeline):
    w = sc.small_gates(T=3, classes={1: 0}, mailboxes=[(64, 37, 1)], stash={0: 4})   # class 1: no stash
    eng = engine_for(w)
    eng.tell(*sc.gate_msgs(wl.GATE_DATA, [1, 2]))
    st = sc.counts(eng.run())
    info, alive = eng.stash_info(), eng.read_state()[1]
    eng.close()
    assert alive[sc.LAST] == 0 and info["overflows"] == 1 and info["stashed"] == 0
    assert st["delivered"] == 1 and st["dead_letters"] == 1 and conserved(st)


# ------------------------------------------------------------------ 9. refusals
def _status(fn):
    with pytest.raises(AgxError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(built):
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    st, msg = _status(lambda: eng.set_stash(0, 4))
    assert st == EINVAL and "n_ranks" in msg
    eng.close()

    eng = GpuEngine(EngineConfig(n_actors=64, n_words=8, max_emit=3))  # a CRDT kind before the call
    eng.register_range(0, 64, Kind.GCOUNTER)
    st, msg = _status(lambda: eng.set_stash(0, 4))
    assert st == EINVAL and "CRDT" in msg
    eng.close()

    eng = GpuEngine(EngineConfig(n_actors=64, n_words=8))              # ... and after it
    eng.set_stash(0, 4)
    st, msg = _status(lambda: eng.register_range(0, 64, Kind.GCOUNTER))
    assert st == EINVAL and "deque-based" in msg
    st, msg = _status(lambda: eng.set_mailbox_priority(0, bytes(256)))  # a priority table after the call
    assert st == EINVAL and "deque-based" in msg
    st, msg = _status(lambda: eng.set_stash(3, 4))                      # an unconfigured class
    assert st == EINVAL and "not configured" in msg
    for cap in (0, 256):
        st, msg = _status(lambda: eng.set_stash(0, cap))
        assert st == EINVAL and "1..255" in msg
    eng.close()

    eng = GpuEngine(EngineConfig(n_actors=64))                          # a priority table before the call
    eng.set_mailbox_priority(0, bytes(256))
    st, msg = _status(lambda: eng.set_stash(0, 4))
    assert st == EINVAL and "priority" in msg
    eng.close()

    w = sc.small_gates()
    eng = engine_for(w)
    eng.tell(*sc.gate_msgs(wl.GATE_DATA, [1]))
    eng.run()
    st, msg = _status(lambda: eng.set_stash(0, 5))                      # after a run
    assert st == ESTATE and "before the first agx_run" in msg
    eng.close()


def test_refused_on_a_ring_pool(built, monkeypatch):
    monkeypatch.setenv("AGX_RADIX_BITS", "3")
    monkeypatch.setenv("AGX_NO_FUSED", "1")
    monkeypatch.setenv("AGX_RING_APPLY", "1")
    from tests.prio_cases import echo_population
    eng = engine_for(echo_population(3, 8))   # bounded FIFO actors without a stash: the per-actor rings come up
    eng.tell(np.arange(8, dtype=np.uint32), 1 << 24)
    eng.run()
    st, msg = _status(lambda: eng.set_stash(0, 4))
    eng.close()
    # (agx_set_stash looks at the ring pool before it looks at `started`: this message means the pool exists)
    assert st == EINVAL and "rings" in msg and "stash" in msg


def test_stash_results_without_a_stash_class(built, pipeline):
    """behaviours that stash on an engine whose classes have no stash capacity: agx_run refuses, loudly"""
    w = sc.small_gates(stash={})
    eng = engine_for(w)
    eng.tell(*sc.gate_msgs(wl.GATE_DATA, [1]))
    st, msg = _status(lambda: eng.run())
    eng.close()
    assert st == EINVAL and "agx_set_stash" in msg


def test_kinds_after_unstash_all(built, pipeline):
    """unstash_all(next) stores the next behaviour: closed -> open on Open, open -> closed on Close"""
    w = sc.small_gates(T=2)
    eng, m = engine_for(w), model_for(w)
    closed, opened = (w.behaviors.kind_of(b) for b in w.behaviors.behaviors[:2])
    for t in (eng, m):
        t.tell(*sc.gate_msgs(wl.GATE_DATA, [1, 2], dst=5))
        t.tell(*sc.gate_msgs(wl.GATE_OPEN, [0], dst=5))      # buffer not empty: released, becomes open
        t.tell(*sc.gate_msgs(wl.GATE_OPEN, [0], dst=6))      # buffer empty: the isEmpty shortcut, becomes open too
        t.tell(*sc.gate_msgs(wl.GATE_OPEN, [0], dst=7))
        t.tell(*sc.gate_msgs(wl.GATE_CLOSE, [0], dst=7))     # ... and closed again
        t.run()
    k = eng.read_kinds()
    eng.close()
    assert k.tolist() == m.read_kinds().tolist()
    assert (k[5], k[6], k[7], k[8]) == (opened, opened, closed, closed)


def _over_tile(stash_target: bool):
    """2049 Close tells to one gate of a 32-actor bucket: bucket 0 holds the stash class, bucket 1 none"""
    w = sc.small_gates(T=5, classes={1: 0}, mailboxes=[(32, 69, 1)], stash={0: 4})
    d, p, s = sc.gate_msgs(wl.GATE_CLOSE, np.arange(2049), dst=7 if stash_target else 40)
    w.tells = (d, s, p)
    return w


def test_over_tile_is_loud(built, pipeline):
    eng = engine_for(_over_tile(True))
    st, msg = _status(lambda: eng.run())
    eng.close()
    assert st == ECAPACITY and "deque-based" in msg and "tile of 2048 messages" in msg


def test_over_tile_other_bucket_unaffected(built, pipeline):
    w = _over_tile(False)
    eng, m = engine_for(w), model_for(w)
    got, exp = sc.counts(eng.run()), sc.counts(m.run())
    eng.close()
    assert got == exp and got["delivered"] == 2049


# ------------------------------------------------------------------ the dispatcher binds its mailbox type's stash
def test_dispatcher_deque_based_mailbox(built):
    from akka_amd.config import Config
    from akka_amd.dispatch import Behavior, Dispatchers, UnboundedDequeBasedMailbox
    conf = Config.parse_string("""
    gpu-dispatcher {
      type = "akka_amd.dispatch.GpuDispatcherConfigurator"
      throughput = 3
      mailbox-type = "akka.dispatch.UnboundedDequeBasedMailbox"
      stash-capacity = 10
      actors = 64
      max-emit = 1
    }""")
    d = Dispatchers(conf).lookup("gpu-dispatcher")
    assert isinstance(d.mailbox_type, UnboundedDequeBasedMailbox) and d.mailbox_type.stash_capacity == 10
    b = sc.kat_behavior("support_unstash_all")
    tb = typed.compile_behaviors([b], max_emit=1)
    d.engine.set_behaviors(tb)
    d.engine.set_outbound(sc.HOST, 1)
    ref = d.spawn(Behavior(tb.kind_of(b), (0, 0)), 64)
    k = sc.KATS["support_unstash_all"]
    p = sc.payloads(k["script"])
    d.tell(np.full(p.size, ref.ref(sc.ACTOR), np.uint32), p)
    d.run()
    assert d.engine.take_outbound()[2].tolist() == sc.payloads(k["expected"]).tolist()
    assert d.engine.stash_info()["stashed"] == k["stashed"]
    d.shutdown()
