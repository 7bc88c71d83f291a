"""Priority and control-aware mailboxes on the GPU (agx_set_mailbox_priority; Mailbox.scala:726-816,
867-1025): the HIP engine through the C ABI against the reference's own known answers, against the
model of DESIGN.md §2.1 (tests/prio_model.py, itself pinned to the frozen oracle by
tests/test_prio_model.py) and -- where the order step must not show -- against the frozen FIFO oracle,
on the fused and the multi-pass pipelines.  The observable for order is the reference specs' own: an
echo behaviour that tells every payload on to a host id (the outbox keeps each sender's order)."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind
from tests import prio_cases as pc
from tests.prio_model import PrioModel, per_sender
from tests.test_prio_model import COUNT_KEYS, run_model, run_oracle, same

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = 1, 5, 6


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as test_mailbox_classes_multipass; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    kw = dict(w.gpu_kwargs(), **cfg)
    eng = GpuEngine(EngineConfig(**kw))
    w.apply_to(eng)
    return eng


def run_gpu(w, max_steps=1 << 30, **cfg):
    eng = engine_for(w, **cfg)
    st = eng.run(max_steps)
    out = eng.take_outbound()
    state = eng.read_state()
    eng.close()
    return {k: getattr(st, k) for k in COUNT_KEYS}, state, out


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


# ------------------------------------------------------------------ 1. stable-priority KAT
@pytest.mark.parametrize("T", pc.KAT_T)
@pytest.mark.parametrize("capacity", pc.KAT_CAPACITY)
def test_stable_priority_kat(built, pipeline, T, capacity):
    w, exp, dead = pc.stable_kat(T, capacity)
    st, _, (d, s, p) = run_gpu(w)
    print("echo", (p >> 24).tolist())
    assert np.array_equal(p, exp)
    assert (s == pc.ECHO_ACTOR).all() and (d == pc.N_KAT).all()
    assert st["dead_letters"] == dead and st["delivered"] == exp.size and st["in_flight"] == 0


# ------------------------------------------------------------------ 2. control-aware KAT
@pytest.mark.parametrize("capacity", [0, 1000])
def test_control_aware_kat(built, pipeline, capacity):
    w, exp = pc.control_kat(capacity)
    assert np.array_equal(run_gpu(w)[2][2], exp)


# ------------------------------------------------------------------ 3. overtaking a backlog
def test_overtake_a_backlog(built, pipeline):
    w = pc.echo_population(2, 0)
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    st, p, normal, control = pc.overtake(eng)
    eng.close()
    mst, mp, _, _ = pc.overtake(PrioModel(**w.engine_kwargs()))
    assert p.tolist() == normal[:2].tolist() + control.tolist() + normal[2:].tolist()
    assert p.tolist() == mp.tolist()
    for k in COUNT_KEYS:
        assert getattr(st, k) == mst[k], k


# ------------------------------------------------------------------ 4. population parity against the model
@pytest.mark.parametrize("bucket_actors", pc.POPULATION_BUCKETS)
@pytest.mark.parametrize("seed,T", pc.POPULATION)
def test_population_parity(built, pipeline, seed, T, bucket_actors):
    w = wl.priority_mix(2048, seed=seed, throughput=T)
    m3 = run_model(w, 3)[1]
    eng = engine_for(w, bucket_actors=bucket_actors)
    s3 = eng.run(3)
    s3 = {k: getattr(s3, k) for k in COUNT_KEYS}
    assert s3 == m3 and conserved(s3) and s3["in_flight"] > 0
    st = eng.run()
    got = ({k: getattr(st, k) for k in COUNT_KEYS}, eng.read_state(), eng.take_outbound())
    eng.close()
    assert conserved(got[0]) and got[0]["in_flight"] == 0
    assert same(got, run_model(w)[1:]) is None


# ------------------------------------------------------------------ 5. the new path against the frozen oracle
@pytest.mark.parametrize("T,C", pc.CONSTANT_TC)
def test_constant_table_equals_oracle(built, pipeline, T, C):
    w = pc.constant_mix(T, C)
    assert same(run_gpu(w, bucket_actors=pc.CONSTANT_BUCKET_ACTORS), run_oracle(w)) is None


# ------------------------------------------------------------------ 6. pre-sorted equivalence
def test_presorted_equals_oracle(built, pipeline):
    w, ref = pc.presorted()
    assert same(run_gpu(w, 1), run_oracle(ref, 1)) is None


# ------------------------------------------------------------------ 7. refusals
def _status(fn):
    with pytest.raises(AgxError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(built):
    tab = pc.control_table()
    eng = GpuEngine(EngineConfig(n_actors=64, n_ranks=2, rank=0))
    st, msg = _status(lambda: eng.set_mailbox_priority(0, tab))
    assert st == EINVAL and "n_ranks" in msg
    eng.close()

    eng = GpuEngine(EngineConfig(n_actors=64, n_words=8, max_emit=3))  # a CRDT kind before the call
    eng.register_range(0, 64, Kind.GCOUNTER)
    st, msg = _status(lambda: eng.set_mailbox_priority(0, tab))
    assert st == EINVAL and "CRDT" in msg
    eng.close()

    eng = GpuEngine(EngineConfig(n_actors=64, n_words=8, max_emit=3))  # ... and after it
    eng.set_mailbox_priority(0, tab)
    st, msg = _status(lambda: eng.register_range(0, 64, Kind.GCOUNTER))
    assert st == EINVAL and "priority" in msg
    st, msg = _status(lambda: eng.set_mailbox_priority(3, tab))  # an unconfigured class
    assert st == EINVAL and "not configured" in msg
    eng.set_mailbox_class(3, 5)
    eng.set_mailbox_priority(3, tab)
    eng.set_mailbox_priority(3, None)  # cleared
    eng.close()

    w = pc.echo_population(5, 0)
    eng = engine_for(w)
    eng.tell(np.arange(8, dtype=np.uint32), 1 << 24)
    eng.run()
    st, msg = _status(lambda: eng.set_mailbox_priority(0, tab))  # after a run
    assert st == ESTATE and "before the first agx_run" in msg
    eng.close()


def _over_tile(prioritised_target: bool):
    """2100 tells to one actor of a 32-actor bucket; class 1 is prioritised, class 0 FIFO"""
    w = pc.echo_population(50, 0)
    w.mailbox_classes = {1: 0}
    w.mailboxes = [(0, 32, 1)]             # bucket 0 holds the prioritised actors, bucket 1 none
    w.mailbox_priorities = {1: pc.control_table()}
    target = 7 if prioritised_target else 40
    pay = ((np.arange(2100, dtype=np.uint32) % 3 + 1) << np.uint32(24)) | np.arange(2100, dtype=np.uint32)
    w.tells = (np.full(2100, target, np.uint32), np.full(2100, 0xFFFFFFFF, np.uint32), pay)
    return w


def test_over_tile_is_loud(built, pipeline):
    eng = engine_for(_over_tile(True))
    st, msg = _status(lambda: eng.run())
    eng.close()
    assert st == ECAPACITY and "tile of 2048 messages" in msg


def test_over_tile_fifo_bucket_unaffected(built, pipeline):
    w = _over_tile(False)
    assert same(run_gpu(w), run_model(w)[1:]) is None


# ------------------------------------------------------------------ the dispatcher binds its mailbox type's table
def test_dispatcher_control_aware_mailbox(built):
    from akka_amd import typed
    from akka_amd.config import Config
    from akka_amd.dispatch import Behavior, Dispatchers, UnboundedControlAwareMailbox
    conf = Config.parse_string("""
    gpu-dispatcher {
      type = "akka_amd.dispatch.GpuDispatcherConfigurator"
      throughput = 5
      mailbox-type = "akka.dispatch.UnboundedControlAwareMailbox"
      gpu.control-tags = [3]
      actors = 64
      max-emit = 1
    }""")
    d = Dispatchers(conf).lookup("gpu-dispatcher")
    assert isinstance(d.mailbox_type, UnboundedControlAwareMailbox)
    e = typed.echo(64)
    tb = typed.compile_behaviors([e], max_emit=1)
    d.engine.set_behaviors(tb)
    d.engine.set_outbound(64, 1)
    ref = d.spawn(Behavior(tb.kind_of(e), (0, 0)), 64)
    _, exp = pc.control_kat(0)
    d.tell(np.full(3, ref.ref(5), np.uint32), np.asarray([1, 2, 3], np.uint32) << np.uint32(24))
    d.run()
    assert np.array_equal(d.engine.take_outbound()[2], exp)
    d.shutdown()
