"""What an LWWMap engine refuses (include/akka_gpu.h "LWWMap replicas"), each with a message, and which
ops an LWWMap replica does not handle."""
import numpy as np
import pytest

from akka_amd._lib import AgxError, check
from akka_amd.engine import CRDT_WORDS, EngineConfig, GpuEngine, Kind, Op
from tests import lwwmap_model as L

pytestmark = pytest.mark.gpu

W = CRDT_WORDS[Kind.LWWMAP]
AGX_EINVAL, AGX_ESTATE = 1, 6


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as in test_gpu_crdt_states.py)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine(n=16, **kw):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, n_words=W, max_emit=3, bucket_actors=32), **kw)))


def refused(status, words, fn):
    with pytest.raises(AgxError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    msg = str(ei.value)
    assert len(msg) > 20 and all(w in msg for w in words), msg


def test_other_kinds_beside_lwwmap(built):
    for other in (Kind.ORSET, Kind.GCOUNTER, Kind.COUNTER, Kind.RING):
        eng = engine()
        eng.register_range(0, 8, Kind.LWWMAP)
        refused(AGX_EINVAL, ["LWWMap", "separate engines"], lambda: eng.register_range(8, 8, other))
        eng.close()
        eng = engine()
        eng.register_range(0, 8, other)
        refused(AGX_EINVAL, ["LWWMap", "separate engines"], lambda: eng.register_range(8, 8, Kind.LWWMAP))
        eng.close()
    eng = engine()
    eng.register_range(0, 16, Kind.LWWMAP)
    eng.register_range(12, 4, Kind.NONE)  # (unregistering stays possible)
    eng.close()


def test_delta_crdt(built):
    eng = engine(n_words=656, max_emit=4)
    eng.register_range(0, 16, Kind.LWWMAP)
    refused(AGX_EINVAL, ["delta-CRDT", "LWWMap"], lambda: eng.set_delta_crdt(50))
    eng.close()
    eng = engine(n_words=656, max_emit=4)
    eng.set_delta_crdt(50)
    refused(AGX_EINVAL, ["delta-CRDT", "LWWMap"], lambda: eng.register_range(0, 16, Kind.LWWMAP))
    eng.close()


def test_more_than_one_rank(built):
    eng = engine(n_ranks=2, rank=0)
    refused(AGX_EINVAL, ["LWWMap", "single-rank"], lambda: eng.register_range(0, 16, Kind.LWWMAP))
    eng.close()


def test_feature_engine(built):
    eng = engine(max_emit=1)  # (timers need max_emit 1)
    eng.set_timers(1)
    refused(AGX_EINVAL, ["CRDT kinds cannot be registered on an engine with"], lambda: eng.register_range(0, 16, Kind.LWWMAP))
    eng.close()


def test_too_few_words(built):
    eng = engine(n_words=355)
    refused(AGX_EINVAL, ["n_words >= 356"], lambda: eng.register_range(0, 16, Kind.LWWMAP))
    eng.close()


def test_set_lwwmap_refusals(built):
    eng = engine()
    refused(AGX_EINVAL, ["no LWWMap replicas"], lambda: eng.set_lwwmap("default", 0))
    eng.register_range(0, 16, Kind.LWWMAP)
    refused(AGX_EINVAL, ["base", "2^62"], lambda: eng.set_lwwmap("default", 1 << 62))
    refused(AGX_EINVAL, ["unknown clock"], lambda: check(eng.lib.agx_set_lwwmap(eng._h, 2, 0)))
    with pytest.raises(ValueError):
        eng.set_lwwmap("wall", 0)
    eng.set_lwwmap("reverse", (1 << 62) - 1)
    eng.set_lwwmap("default", 5)
    eng.tell([0], [Op.put(1, 2)])
    eng.run()
    refused(AGX_ESTATE, ["before the first agx_run"], lambda: eng.set_lwwmap("default", 5))
    words, _ = eng.read_state()
    assert L.from_words(words[0]).values[1] == (0, 2, 6)
    eng.close()


def test_ops_an_lwwmap_replica_does_not_handle(built, pipeline):
    """PUT with key 63 is handled; REMOVE of key 64 (and beyond) is unhandled -- a PUT's key is the low six
    bits of its argument, so Op.put refuses key 64 before it reaches the engine; INCREMENT, DECREMENT, ADD,
    CLEAR, DELTA_TICK and an unknown op are Behaviors.unhandled and leave the state alone."""
    with pytest.raises(ValueError):
        Op.put(64, 1)
    eng = engine()
    eng.register_range(0, 16, Kind.LWWMAP)
    eng.set_gossip(2, 3)
    eng.tell([5], [Op.put(63, 7)])
    st = eng.run()
    assert st.unhandled == 0 and st.delivered == 1
    before, _ = eng.read_state()
    assert L.from_words(before[5]).entries == {63: 7}
    bad = [Op.make(Op.REMOVE, 64), Op.make(Op.REMOVE, 0xFFFFFF), Op.make(Op.INCREMENT, 1), Op.make(Op.DECREMENT, 1),
           Op.make(Op.ADD, 63), Op.make(Op.CLEAR), Op.make(Op.DELTA_TICK, 0), Op.make(9, 1), Op.make(0, 3), Op.make(255, 0)]
    eng.tell([5] * len(bad), bad)
    st2 = eng.run()
    assert st2.unhandled - st.unhandled == len(bad) and st2.delivered - st.delivered == len(bad)
    assert st2.emitted == st.emitted and st2.in_flight == 0
    after, _ = eng.read_state()
    assert np.array_equal(before, after)
    eng.close()


def test_compiled_behaviours_beside_lwwmap(built):
    eng = engine()
    eng.register_range(0, 8, Kind.LWWMAP)
    refused(AGX_EINVAL, ["separate engines"], lambda: eng.register_range(8, 8, 16))  # (AGX_KIND_COMPILED + 0)
    eng.close()
