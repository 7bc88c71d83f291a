"""What agx_set_lwwmap_delta refuses (include/akka_gpu.h "LWWMap delta replication"), each with its status and the
words of its message; agx_set_delta_crdt stays refused on such an engine; and an LWWMap engine without the call
behaves as before: AGX_OP_DELTA_TICK is Behaviors.unhandled there."""
import numpy as np
import pytest

from akka_amd._lib import AgxError
from akka_amd.engine import CRDT_WORDS, LWWMAP_DELTA_WORDS, EngineConfig, GpuEngine, Kind, Op
from tests import lwwmap_model as L

pytestmark = pytest.mark.gpu

W = LWWMAP_DELTA_WORDS
AGX_EINVAL, AGX_ESTATE = 1, 6


def engine(n=16, **kw):
    return GpuEngine(EngineConfig(**dict(dict(n_actors=n, n_words=W, max_emit=4, bucket_actors=32), **kw)))


def refused(status, words, fn):
    with pytest.raises(AgxError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    msg = str(ei.value)
    assert len(msg) > 20 and all(w in msg for w in words), msg


def test_no_lwwmap_replicas(built):
    eng = engine()
    refused(AGX_EINVAL, ["agx_set_lwwmap_delta", "no LWWMap replicas"], lambda: eng.set_lwwmap_delta(50))
    eng.register_range(0, 16, Kind.ORSET)
    refused(AGX_EINVAL, ["agx_set_lwwmap_delta", "no LWWMap replicas"], lambda: eng.set_lwwmap_delta(50))
    eng.close()


@pytest.mark.parametrize("m", [0, 51, 1 << 20])
def test_max_delta_size_out_of_range(built, m):
    eng = engine()
    eng.register_range(0, 16, Kind.LWWMAP)
    refused(AGX_EINVAL, ["max_delta_size", "1..50"], lambda: eng.set_lwwmap_delta(m))
    eng.set_lwwmap_delta(1)
    eng.set_lwwmap_delta(50)  # (the bounds themselves are fine, and the call may be repeated before the first run)
    eng.close()


def test_max_emit_below_4(built):
    eng = engine(max_emit=3)
    eng.register_range(0, 16, Kind.LWWMAP)
    refused(AGX_EINVAL, ["max_emit >= 4"], lambda: eng.set_lwwmap_delta(50))
    eng.close()


def test_more_than_one_rank(built):
    eng = engine(n_ranks=2, rank=0)
    refused(AGX_EINVAL, ["agx_set_lwwmap_delta", "single-rank"], lambda: eng.set_lwwmap_delta(50))
    eng.close()


@pytest.mark.parametrize("words", [CRDT_WORDS[Kind.LWWMAP], W - 1])
def test_too_few_words(built, words):
    eng = engine(n_words=words)
    eng.register_range(0, 16, Kind.LWWMAP)
    refused(AGX_EINVAL, ["n_words >= 880"], lambda: eng.set_lwwmap_delta(50))
    eng.close()


def test_after_the_first_run(built):
    eng = engine()
    eng.register_range(0, 16, Kind.LWWMAP)
    eng.set_gossip(1, 1)
    eng.tell([0], [Op.put(3, 4)])
    eng.run()
    refused(AGX_ESTATE, ["before the first agx_run"], lambda: eng.set_lwwmap_delta(50))
    eng.close()


def test_set_delta_crdt_stays_refused(built):
    eng = engine()
    eng.register_range(0, 16, Kind.LWWMAP)
    eng.set_lwwmap_delta(50)
    refused(AGX_EINVAL, ["delta-CRDT", "LWWMap"], lambda: eng.set_delta_crdt(50))
    eng.close()


def test_delta_tick_is_unhandled_without_the_call(built):
    """An LWWMap engine that never called set_lwwmap_delta -- even one wide enough for it: the tick is unhandled,
    nothing is told, and the put beside it lands as on any LWWMap engine, the words behind the data untouched."""
    for words in (CRDT_WORDS[Kind.LWWMAP], W):
        eng = engine(n_words=words)
        eng.register_range(0, 16, Kind.LWWMAP)
        eng.set_gossip(1, 1)
        eng.tell([2, 2], [Op.make(Op.DELTA_TICK, 3), Op.put(5, 6)])
        st = eng.run()
        state, _ = eng.read_state()
        eng.close()
        assert (st.unhandled, st.delivered, st.emitted, st.in_flight) == (1, 2, 0, 0)
        want = L.LWWMap().put(2, 5, 6, L.default_clock, 1)
        assert np.array_equal(state[2, :356], L.to_words(want)) and not state[:, 356:].any()
