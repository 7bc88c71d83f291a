"""Pub-sub topics on the GPU (agx_set_topics): the HIP engine through the C ABI against the known
answers restated from the reference's spec (tests/golden/topic_kats.json) and against the model
(tests/topic_model.py), on the fused and the multi-pass pipelines, with graph replays and eager launches.  Everything
is compared bit for bit after every run: states, alive flags, kinds, every counter, receptionist_info, topic_info,
listings, masks, the pending log, the outbox order, and conservation."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine
from tests import topic_cases as tc
from tests.receptionist_model import ReceptionistModel
from tests.topic_model import TopicModel

pytestmark = pytest.mark.gpu

ECAPACITY = 5
TILE_TEXT = ("a bucket of {} actors of an engine with the receptionist received more than one tile of 2048 messages (backlog "
             "included): the launches for larger inboxes know no receptionist (smaller agx_cfg.bucket_actors spread the load)")


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the receptionist fixture)
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
    m = TopicModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def refusal(call):
    """(status, message) of the refusal"""
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]


def both(w, script, n_keys=2):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run"""
    eng, mod = engine_for(w), model_for(w)
    n, sm, m = 0, None, None
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = tc.counts(sg), tc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = tc.snapshot(eng, n_keys), tc.snapshot(mod, n_keys)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert tc.conserved(sg, g["topic_info"])
        n += 1
    eng.close()
    return sm, m


# ------------------------------------------------------------------ 1. the known answers (64 actors, one bucket)
@pytest.mark.parametrize("T", tc.KAT_T)
@pytest.mark.parametrize("name", tc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(tc.node_workload(T))
    got = tc.run_kat(name, eng)
    eng.close()
    print(got)
    tc.check_kat(name, got)
    assert got == tc.run_kat(name, model_for(tc.node_workload(T)))


# ------------------------------------------------------------------ 2. the inbox order, four buckets of 64
def test_order(built, pipeline, launch):
    st, snap = both(tc.order_workload(), tc.order_script)
    assert snap["topic_info"] == dict(published=4, fanned_out=36, no_subscribers=0, host_published=0)
    assert snap["words"][63] == [6 - 2, 250]  # four Notes; the last came from publisher 250


# ------------------------------------------------------------------ 3. membership timing
def test_membership_timing(built, pipeline, launch):
    st, snap = both(tc.timing_workload(), tc.timing_script)
    assert snap["log"] == [] and snap["topic_info"]["no_subscribers"] == 0 and snap["alive"][141] == 0


# ------------------------------------------------------------------ 4. bounded mailboxes
def test_bounded_mailboxes(built, pipeline, launch):
    st, snap = both(tc.bounded_workload(), tc.bounded_script)
    assert st["dead_letters"] == 256 and snap["topic_info"]["fanned_out"] == 6 * 128


# ------------------------------------------------------------------ 5. run budgets between publish and delivery
def test_budgets(built, pipeline, launch):
    w = tc.node_workload(3, n=256, starts=[(60, 11, 0), (200, 1, 1)])
    eng = engine_for(w)
    tc.tells(eng, (5, "PubF:1"))
    st = eng.run(1)
    assert st.in_flight == 11 and st.supersteps == 1  # planned, not yet drained: the engine is not quiescent ...
    st = eng.run()
    assert st.in_flight == 0 and st.supersteps == 2 and st.delivered == 12  # ... the next run delivers
    assert eng.run().supersteps == 2
    eng.close()
    both(w, tc.budget_script)


# ------------------------------------------------------------------ 6. publications from the host
def test_host_publish(built, pipeline, launch):
    st, snap = both(tc.order_workload(), tc.host_publish_script)
    assert snap["topic_info"] == dict(published=2, fanned_out=12 * 5 + 6 * 2, no_subscribers=0, host_published=5)


# ------------------------------------------------------------------ 7. the tile and the log capacity
def test_one_publication_to_a_full_bucket_is_exactly_one_tile(built, pipeline):
    w = tc.node_workload(3, n=4096, bucket_actors=2048, starts=[(2048, 2048, 0)])  # bucket 1 fully subscribed

    def script(t):
        tc.tells(t, (5, "PubF:1"))
        yield t.run()
    st, snap = both(w, script)
    assert st["delivered"] == 1 + 2048 and snap["words"][2048] == [1, 5] and snap["words"][4095] == [1, 5]


def test_one_tell_more_than_a_tile(built, pipeline):
    w = tc.node_workload(3, n=4096, bucket_actors=2048, starts=[(2048, 2048, 0)])
    eng = engine_for(w)
    tc.tells(eng, (5, "PubF:1"))
    eng.run(1)
    tc.tells(eng, (3000, "Ping:1"))
    text = TILE_TEXT.format(2048)
    assert refusal(eng.run) == (ECAPACITY, text)
    assert refusal(eng.run) == (ECAPACITY, text)  # sticky
    eng.close()


def test_33_publications_to_a_full_bucket_of_64(built, pipeline):
    w = tc.node_workload(1, n=256, starts=[(64, 64, 0)])
    eng = engine_for(w)
    tc.tells(eng, *[(a, f"PubF:{a}") for a in range(32)])  # 32 x 64: exactly one tile
    st = eng.run()
    assert st.delivered == 32 + 2048 and eng.topic_info()["fanned_out"] == 2048
    tc.tells(eng, *[(a, f"PubF:{a}") for a in range(33)])
    assert refusal(eng.run) == (ECAPACITY, TILE_TEXT.format(64))
    eng.close()


def test_log_capacity(built, pipeline):
    w = tc.node_workload(1, n=64, log_capacity=4, starts=[(0, 4, 0)])
    eng = engine_for(w)
    tc.tells(eng, *[(a, f"PubF:{a}") for a in range(10, 14)])  # exactly `log_capacity` publications: no error
    st = eng.run()
    assert st.delivered == 4 + 16
    tc.tells(eng, *[(a, f"PubF:{a}") for a in range(10, 15)])
    text = ("a tick's publications would exceed the topics' log capacity of 4 entries (agx_set_topics): the publications "
            "past it are lost")
    assert refusal(eng.run) == (ECAPACITY, text)
    assert refusal(eng.run) == (ECAPACITY, text)  # sticky
    eng.close()


# ------------------------------------------------------------------ 8. the differential workload
@pytest.mark.parametrize("bucket_actors", [64, 2048])
@pytest.mark.parametrize("seed", tc.MESH_SEEDS)
def test_topic_mesh(built, pipeline, launch, seed, bucket_actors):
    w = tc.mesh_workload(seed, bucket_actors)
    st, snap = both(w, tc.mesh_script(w), n_keys=8)
    assert snap["topic_info"]["fanned_out"] > 0 and snap["topic_info"]["no_subscribers"] > 0


# ------------------------------------------------------------------ 9. topics set, nothing published
def test_nothing_published_equals_the_receptionist(built, pipeline, launch):
    """a plain receptionist workload on an engine with topics set equals the same run without agx_set_topics"""
    w = wl.service_mesh(1024, 8, 1, 12)
    plain, topical = engine_for(w), engine_for(w)
    # (set_topics comes after the workload's receptionist calls and before the first run)
    topical.set_topics(16)
    mod = ReceptionistModel(**w.engine_kwargs())
    w.apply_to(mod)
    from tests import receptionist_cases as rc
    for dst, src, pay in w.schedule:
        for t in (plain, topical, mod):
            t.tell(dst, pay, src)
        sp, stt, sm = (rc.counts(t.run(1)) for t in (plain, topical, mod))
        assert sp == stt == sm
    sp, stt = rc.counts(plain.run()), rc.counts(topical.run())
    assert sp == stt
    a, b = rc.snapshot(plain, 8), rc.snapshot(topical, 8)
    for k in a:
        assert a[k] == b[k], k
    assert topical.topic_info() == dict(published=0, fanned_out=0, no_subscribers=0, host_published=0)
    assert np.asarray(topical.read_topic_log()).size == 0
    plain.close()
    topical.close()
