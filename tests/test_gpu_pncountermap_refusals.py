"""What a PNCounterMap engine refuses (include/akka_gpu.h "PNCounterMap replicas"), each with a message,
and which ops a PNCounterMap replica does not handle."""
import numpy as np
import pytest

from akka_amd._lib import AgxError
from akka_amd.engine import CRDT_WORDS, EngineConfig, GpuEngine, Kind, Op
from tests import pncountermap_model as P

pytestmark = pytest.mark.gpu

W = CRDT_WORDS[Kind.PNCOUNTERMAP]
AGX_EINVAL = 1
WIDE = 0x80000000


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as in test_gpu_lwwmap_refusals.py)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine(n=16, **kw):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, n_words=W, max_emit=3, bucket_actors=32, msg_capacity=1024), **kw)))


def refused(status, words, fn):
    with pytest.raises(AgxError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    msg = str(ei.value)
    assert len(msg) > 20 and all(w in msg for w in words), msg


def test_other_kinds_beside_pncountermap(built):
    """Another kind beside it, LWWMap included, in either call order."""
    for other in (Kind.LWWMAP, Kind.ORSET, Kind.PNCOUNTER, Kind.COUNTER, Kind.RING):
        eng = engine()
        eng.register_range(0, 8, Kind.PNCOUNTERMAP)
        refused(AGX_EINVAL, ["PNCounterMap", "separate engines"], lambda: eng.register_range(8, 8, other))
        eng.close()
        eng = engine()
        eng.register_range(0, 8, other)
        refused(AGX_EINVAL, ["PNCounterMap", "separate engines"], lambda: eng.register_range(8, 8, Kind.PNCOUNTERMAP))
        eng.close()
    eng = engine()
    eng.register_range(0, 16, Kind.PNCOUNTERMAP)
    eng.register_range(12, 4, Kind.NONE)  # (unregistering stays possible)
    eng.close()


def test_compiled_behaviours_beside_pncountermap(built):
    eng = engine()
    eng.register_range(0, 8, Kind.PNCOUNTERMAP)
    refused(AGX_EINVAL, ["separate engines"], lambda: eng.register_range(8, 8, 16))  # (AGX_KIND_COMPILED + 0)
    eng.close()


def test_delta_crdt(built):
    eng = engine(max_emit=4)
    eng.register_range(0, 16, Kind.PNCOUNTERMAP)
    refused(AGX_EINVAL, ["delta-CRDT", "PNCounterMap"], lambda: eng.set_delta_crdt(50))
    eng.close()
    eng = engine(max_emit=4)
    eng.set_delta_crdt(50)
    refused(AGX_EINVAL, ["delta-CRDT", "PNCounterMap"], lambda: eng.register_range(0, 16, Kind.PNCOUNTERMAP))
    eng.close()


def test_more_than_one_rank(built):
    eng = engine(n_ranks=2, rank=0)
    refused(AGX_EINVAL, ["PNCounterMap", "single-rank"], lambda: eng.register_range(0, 16, Kind.PNCOUNTERMAP))
    eng.close()


def test_feature_engine(built):
    eng = engine(max_emit=1)  # (timers need max_emit 1)
    eng.set_timers(1)
    refused(AGX_EINVAL, ["CRDT kinds cannot be registered on an engine with"], lambda: eng.register_range(0, 16, Kind.PNCOUNTERMAP))
    eng.close()


def test_too_few_words(built):
    eng = engine(n_words=1295)
    refused(AGX_EINVAL, ["n_words >= 1296"], lambda: eng.register_range(0, 16, Kind.PNCOUNTERMAP))
    eng.close()
    with pytest.raises(AgxError) as ei:  # (1296 is the widest layout)
        engine(n_words=1297)
    assert ei.value.status == AGX_EINVAL and "1296" in str(ei.value)


def test_ops_a_pncountermap_replica_does_not_handle(built, pipeline):
    """INCREMENT and DECREMENT take every 24-bit argument and REMOVE keys below 64; REMOVE of key 64 (and beyond),
    ADD, CLEAR, PUT, DELTA_TICK and an unknown op are Behaviors.unhandled and leave the state alone.  A state
    gossip of data type 0..2 cannot reach a replica: the engine holds no other kind, and the host may not tell
    with a wide sender."""
    eng = engine()
    eng.register_range(0, 16, Kind.PNCOUNTERMAP)
    eng.set_gossip(2, 3)
    eng.tell([5, 5], [Op.make(Op.INCREMENT, 0xFFFFFF), Op.make(Op.DECREMENT, 0xFFFFFF)])
    st = eng.run()
    assert st.unhandled == 0 and st.delivered == 2
    before, _ = eng.read_state()
    assert P.from_words(before[5]).entries == {63: 0} and P.from_words(before[5]).values[63][5] == (1 << 18) - 1
    bad = [Op.make(Op.REMOVE, 64), Op.make(Op.REMOVE, 0xFFFFFF), Op.make(Op.ADD, 63), Op.make(Op.CLEAR), Op.put(3, 4),
           Op.make(Op.DELTA_TICK, 0), Op.make(9, 1), Op.make(0, 3), Op.make(255, 0)]
    eng.tell([5] * len(bad), bad)
    st2 = eng.run()
    assert st2.unhandled - st.unhandled == len(bad) and st2.delivered - st.delivered == len(bad)
    assert st2.emitted == st.emitted and st2.in_flight == 0
    after, _ = eng.read_state()
    assert np.array_equal(before, after)
    for t in range(3):
        refused(AGX_EINVAL, ["not an actor id"], lambda: eng.tell([5], [t << 30], src=[WIDE | 4]))
    eng.close()
