"""What an ORMultiMap engine refuses (include/akka_gpu.h "ORMultiMap replicas"), each with a message."""
import numpy as np
import pytest

from akka_amd._lib import AgxError
from akka_amd.engine import CRDT_WORDS, EngineConfig, GpuEngine, Kind, Op
from tests import ormultimap_model as P

pytestmark = pytest.mark.gpu

W = CRDT_WORDS[Kind.ORMULTIMAP]
AGX_EINVAL = 1
WIDE = 0x80000000


def engine(n=16, **kw):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, n_words=W, max_emit=3, bucket_actors=32, msg_capacity=1024), **kw)))


def refused(status, words, fn):
    with pytest.raises(AgxError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    msg = str(ei.value)
    assert len(msg) > 20 and all(w in msg for w in words), msg


def test_other_kinds_beside_ormultimap(built):
    """Another kind beside it, the other two maps included, in either call order."""
    for other in (Kind.PNCOUNTERMAP, Kind.LWWMAP, Kind.ORSET, Kind.PNCOUNTER, Kind.COUNTER, Kind.RING):
        eng = engine()
        eng.register_range(0, 8, Kind.ORMULTIMAP)
        refused(AGX_EINVAL, ["ORMultiMap", "separate engines"], lambda: eng.register_range(8, 8, other))
        eng.close()
        eng = engine()
        eng.register_range(0, 8, other)
        refused(AGX_EINVAL, ["ORMultiMap", "separate engines"], lambda: eng.register_range(8, 8, Kind.ORMULTIMAP))
        eng.close()
    eng = engine()
    eng.register_range(0, 16, Kind.ORMULTIMAP)
    eng.register_range(12, 4, Kind.NONE)  # (unregistering stays possible)
    eng.close()


def test_compiled_behaviours_beside_ormultimap(built):
    eng = engine()
    eng.register_range(0, 8, Kind.ORMULTIMAP)
    refused(AGX_EINVAL, ["ORMultiMap", "separate engines"], lambda: eng.register_range(8, 8, 16))  # (AGX_KIND_COMPILED + 0)
    eng.close()


def test_delta_crdt(built):
    eng = engine(max_emit=4)
    eng.register_range(0, 16, Kind.ORMULTIMAP)
    refused(AGX_EINVAL, ["delta-CRDT", "ORMultiMap"], lambda: eng.set_delta_crdt(50))
    eng.close()
    eng = engine(max_emit=4)
    eng.set_delta_crdt(50)
    refused(AGX_EINVAL, ["delta-CRDT", "ORMultiMap"], lambda: eng.register_range(0, 16, Kind.ORMULTIMAP))
    eng.close()


def test_more_than_one_rank(built):
    eng = engine(n_ranks=2, rank=0)
    refused(AGX_EINVAL, ["ORMultiMap", "single-rank"], lambda: eng.register_range(0, 16, Kind.ORMULTIMAP))
    eng.close()


def test_other_state_widths(built):
    for nw in (CRDT_WORDS[Kind.PNCOUNTERMAP], CRDT_WORDS[Kind.ORSET], 2):
        eng = engine(n_words=nw)
        refused(AGX_EINVAL, ["ORMultiMap", "n_words = 2576"], lambda: eng.register_range(0, 16, Kind.ORMULTIMAP))
        eng.close()
    # 2576 is the widest layout, and the only width above the 1296 of every other engine
    for nw in (W + 1, W - 1, CRDT_WORDS[Kind.PNCOUNTERMAP] + 1, 2000):
        with pytest.raises(AgxError) as ei:
            engine(n_words=nw)
        assert ei.value.status == AGX_EINVAL and "2576" in str(ei.value) and "1296" in str(ei.value) and "ORMultiMap" in str(ei.value)


def test_state_gossip_of_another_type_through_the_host(built):
    """A state gossip of data type 0..2 cannot reach a replica: the engine holds no other kind, and the host may
    not tell with a wide sender.  The state stays as it was."""
    eng = engine()
    eng.register_range(0, 16, Kind.ORMULTIMAP)
    eng.set_gossip(2, 3)
    eng.tell([5], [Op.put_set(9, [0, 7])])
    st = eng.run()
    before, _ = eng.read_state()
    assert st.unhandled == 0 and P.from_words(before[5]).entries == {9: frozenset({0, 7})}
    for t in range(3):
        refused(AGX_EINVAL, ["not an actor id"], lambda: eng.tell([5], [t << 30], src=[WIDE | 4]))
    st2 = eng.run()
    after, _ = eng.read_state()
    assert st2.delivered == st.delivered and np.array_equal(before, after)
    eng.close()
