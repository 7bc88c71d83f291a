"""Subscribe / Find and the Listing message on the GPU (agx_set_listings): the HIP engine through the C
ABI against the known answers restated from the reference's spec (tests/golden/listing_kats.json) and against the model
(tests/listing_model.py), on the fused and the multi-pass pipelines, with graph replays and eager launches.  Everything
is compared bit for bit after every run: states, alive flags, kinds, every counter, receptionist_info, topic_info,
listing_info, listings, the three masks, the pending log, the outbox order, and conservation."""
import pytest

from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine
from tests import listing_cases as lc
from tests.listing_model import ListingModel

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
    m = ListingModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def refusal(call):
    """(status, message) of the refusal"""
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]


def both(w, script):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run; the last stats, the last snapshot and every report"""
    eng, mod = engine_for(w), model_for(w)
    n, sm, m, reports = 0, None, None, {}
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = lc.counts(sg), lc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = lc.snapshot(eng), lc.snapshot(mod)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert lc.conserved(sg, g["topic_info"], g["listing_info"])
        for a, r in lc.reports_of(g).items():
            reports.setdefault(a, []).extend(r)
        n += 1
    eng.close()
    return sm, m, reports


def listings_of(reports, a):
    return [r[1:] for r in reports.get(a, []) if r[0] == "L"]


# ------------------------------------------------------------------ 1. the known answers (64 actors, one bucket)
@pytest.mark.parametrize("T", lc.KAT_T)
@pytest.mark.parametrize("name", lc.KAT_NAMES)
def test_kat(built, pipeline, launch, name, T):
    eng = engine_for(lc.node_workload(T))
    got = lc.run_kat(name, eng)
    eng.close()
    print(got)
    lc.check_kat(name, got)
    assert got == lc.run_kat(name, model_for(lc.node_workload(T)))


# ------------------------------------------------------------------ 2. order and boundaries: 250 actors in buckets of 64
def test_order_and_boundaries(built, pipeline, launch):
    st, snap, rep = both(lc.order_workload(), lc.order_script)
    # an arrival, a host-staged tell, the publication, then the Listings in ascending key
    assert rep[64] == [("L", 0, 1), ("L", 1, 1), ("G", 64), ("G", 8), ("G", 9), ("L", 0, 2), ("L", 1, 0)]
    for a in (63, 127, 128, 191, 192, 249):  # both sides of every boundary and the end of the short bucket
        assert listings_of(rep, a)[-1] == ((0, 2) if a not in (63,) else (1, 0)), a
    assert snap["words"][249] == [2, 5]


def test_a_subscriber_with_backlog(built, pipeline, launch):
    st, snap, rep = both(lc.order_workload(1), lc.backlog_script)
    assert rep[64][-5:] == [("G", 1), ("G", 2), ("G", 3), ("L", 0, 3), ("L", 0, 3)]


# ------------------------------------------------------------------ 3. timing
def test_timing(built, pipeline, launch):
    st, snap, rep = both(lc.timing_workload(), lc.timing_script)
    assert listings_of(rep, 20) == [(0, 2), (0, 1), (0, 1)] and listings_of(rep, 21) == [(1, 0)]
    assert listings_of(rep, 22) == [(0, 2)] and listings_of(rep, 70) == [(0, 1), (0, 2), (0, 1)]
    assert listings_of(rep, 140) == [(0, 1), (0, 2)] and listings_of(rep, 23) == []
    assert snap["info"]["version"][1] == 0 and snap["sub"][23] == 0 and snap["pending"][23] == 0


# ------------------------------------------------------------------ 4. bounded mailboxes
def test_bounded_mailboxes(built, pipeline, launch):
    st, snap, rep = both(lc.bounded_workload(), lc.bounded_script)
    assert st["dead_letters"] == 128 and snap["listing_info"]["listings_sent"] == 4 * 128
    assert listings_of(rep, 64) == [(0, 0), (1, 1), (0, 1)]


# ------------------------------------------------------------------ 5. run budgets between a change and its Listings
def test_budgets(built, pipeline, launch):
    w = lc.order_workload()
    eng = engine_for(w)
    eng.run()
    lc.tells(eng, (7, "Reg:0"))
    st = eng.run(1)
    assert st.in_flight == 7 and st.supersteps == 2  # owed, not yet drained: the engine is not quiescent ...
    assert eng.listing_info()["listings_sent"] == 10 + 7
    st = eng.run()
    assert st.in_flight == 0 and st.supersteps == 3  # ... the next run delivers
    assert eng.run().supersteps == 3                 # ... and a third does nothing
    eng.close()
    both(w, lc.budget_script)


# ------------------------------------------------------------------ 6. host calls between runs
def test_host_calls(built, pipeline, launch):
    st, snap, rep = both(lc.order_workload(), lc.host_calls_script)
    assert listings_of(rep, 100) == [(0, 1), (0, 3), (0, 5), (0, 7)]
    assert listings_of(rep, 64) == [(0, 1), (1, 1), (0, 3), (0, 5), (0, 7), (1, 2), (1, 3)]


# ------------------------------------------------------------------ 7. the seeded random mesh
@pytest.mark.parametrize("n,bucket_actors", [(256, 64), (256, 256), (1024, 64), (1024, 256)])
@pytest.mark.parametrize("seed", lc.MESH_SEEDS)
def test_mesh(built, pipeline, launch, seed, n, bucket_actors):
    w = lc.mesh_workload(seed, n, bucket_actors)
    st, snap, rep = both(w, lc.mesh_script(w))
    li = snap["listing_info"]
    assert li["listings_sent"] > li["subscribes"] and li["notified"] > 0


# ------------------------------------------------------------------ 8. the tile limit
def test_two_keys_to_a_full_bucket_exceed_the_tile(built, pipeline, launch):
    eng = engine_for(lc.tile_workload())
    g = lc.tile_script(2)(eng)
    assert next(g).delivered == 2048 and next(g).delivered == 4096
    text = TILE_TEXT.format(2048)
    assert refusal(lambda: next(g)) == (ECAPACITY, text)  # 2 x 2048 Listings in one tick
    assert refusal(eng.run) == (ECAPACITY, text)  # sticky
    eng.close()


def test_one_key_to_a_full_bucket_is_one_tile(built, pipeline, launch):
    st, snap, rep = both(lc.tile_workload(), lc.tile_script(1))
    assert snap["words"][2047] == [3, 5] and snap["listing_info"]["listings_sent"] == 3 * 2048
    assert st["delivered"] == 3 * 2048 + 1
