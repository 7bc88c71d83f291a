"""Sharded entities on the GPU (agx_set_sharding; akka-cluster-sharding Shard.scala:388-516): the HIP engine through the
C ABI against the known answers worked out by hand from Shard.scala (tests/golden/sharding_kats.json; no JVM is
available to record them) and against the model of DESIGN.md §2.13 (tests/sharding_model.py, itself pinned to the
known answers and to the receive timeouts' model by tests/test_sharding_model.py), on the fused and the multi-pass
pipelines.  Populations of 80 ids in buckets of 32 (a partial last bucket) with two entity types that straddle a bucket
boundary beside registered plain actors; the seeded workloads hold 96 to 200 entities.  The observable for order is an
echo to a host id (the outbox keeps each sender's order)."""
import numpy as np
import pytest

from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine
from tests import sharding_cases as sc
from tests.sharding_model import ShardingModel

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the receive timeouts' fixture; NO_FUSED: populations of one digit)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))
    w.apply_to(eng)
    return eng


def model_for(w):
    m = ShardingModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def diff(g, m):
    return {k: (g[k], m[k]) for k in g if g[k] != m[k]}


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(sc.scenario_workload(name, T))
    got = sc.run_kat(name, T, eng)
    eng.close()
    print(got)
    sc.check_kat(name, T, got)
    assert got == sc.run_kat(name, T, model_for(sc.scenario_workload(name, T)))


# ------------------------------------------------------------------ 2. the seeded workloads, tick by tick
@pytest.mark.parametrize("name", list(sc.seeded_workloads()))
def test_workload_tick_by_tick(built, pipeline, name):
    """after every tick: counters, sharding_info, read_entities, receive-timeout rows, state words, alive flags, echo"""
    w = sc.seeded_workloads()[name]
    eng, mod = engine_for(w), model_for(w)
    t = 0
    for dst, src, pay in w.schedule:
        for target in (eng, mod):
            if len(dst):
                target.tell(dst, pay, src)
        g, m = sc.snapshot(eng, eng.run(1)), sc.snapshot(mod, mod.run(1))
        assert g == m, (name, t, diff(g, m))
        t += 1
    while m["counts"]["in_flight"] or m["rt_info"]["pending"]:
        g, m = sc.snapshot(eng, eng.run(1)), sc.snapshot(mod, mod.run(1))
        assert g == m, (name, t, diff(g, m))
        t += 1
        assert t < 200
    g, m = sc.snapshot(eng, eng.run()), sc.snapshot(mod, mod.run())
    eng.close()
    assert g == m and g["info"]["alive"] == 0 and g["info"]["restarted"] > 0 and g["counts"]["in_flight"] == 0


# ------------------------------------------------------------------ 3. run(1) x n equals run(n)
@pytest.mark.parametrize("name, n", [("sharded_entities_T1", 5), ("passivation_race_T16", 3)])
def test_split_run_equals_one_run(built, pipeline, name, n):
    """n ticks, short of quiescence: both runs end by their budget, with mail queued and entities passivating"""
    w = sc.seeded_workloads()[name]
    a, b = engine_for(w), engine_for(w)
    dst, src, pay = (np.concatenate([s[i] for s in w.schedule[:3]]) for i in range(3))
    for eng in (a, b):
        eng.tell(dst, pay, src)
    for _ in range(n):
        sa = a.run(1)
    sb = b.run(n)
    ga, gb = sc.snapshot(a, sa), sc.snapshot(b, sb)
    a.close(), b.close()
    assert ga == gb and ga["timer_info"]["ticks"] == n and ga["info"]["started"] > 0
    assert ga["counts"]["in_flight"] > 0 and sum(ga["entities"]["passivating"]) > 0


# ------------------------------------------------------------------ 4. a random script on the 80-id population
@pytest.mark.parametrize("T", [1, 3])
def test_random_script(built, pipeline, T):
    """40 ticks of jobs, forwards, passivates, plain stops, self-tells and timers to both entity types, the plain
    actors and two unknown ids, against the model after every tick"""
    rng = np.random.default_rng(40 + T)
    menu = ["Job", "Job", "Job", "Passivate", "Stop", "SelfTell", "SelfStop", "Arm", "Bye", "Fwd:30", "Fwd:55", "Fwd:33"]
    eng, mod = engine_for(sc.kat_workload(T, capacity=4)), model_for(sc.kat_workload(T, capacity=4))
    for t in range(40):
        k = int(rng.integers(0, 14))
        dst = rng.integers(0, sc.N_KAT + 2, k).astype(np.uint32)   # (ids 80, 81: the host and an unknown ref)
        dst[dst == sc.HOST] = 33
        pay = np.asarray([sc.payload(menu[int(i)]) for i in rng.integers(0, len(menu), k)], np.uint32)
        for target in (eng, mod):
            if k:
                target.tell(dst, pay, np.full(k, NO_SENDER, np.uint32))
        g, m = sc.snapshot(eng, eng.run(1)), sc.snapshot(mod, mod.run(1))
        assert g == m, (T, t, diff(g, m))
    eng.close()
    i = g["info"]
    assert i["started"] > 10 and i["passivated"] > 0 and i["passivate_unknown"] > 0 and g["counts"]["dead_letters"] > 0


# ------------------------------------------------------------------ 5. a bucket of entities without mail, and one of plain actors
def test_idle_buckets_and_plain_buckets(built, pipeline):
    """mail for the plain actors of bucket 0 only: the entity buckets run their tick without a start; then one job in
    the partial last bucket's neighbour starts exactly one entity"""
    w = sc.kat_workload(3)
    eng, mod = engine_for(w), model_for(w)
    got = []
    for target in (eng, mod):
        sc.tell_pairs(target, [(1, "Job"), (2, "Job")])
        a = sc.snapshot(target, target.run())
        sc.tell_pairs(target, [(69, "Job")])
        b = sc.snapshot(target, target.run(1))
        got.append((a, b))
        target.close()
    assert got[0] == got[1]
    a, b = got[0]
    assert a["info"]["started"] == 0 and sum(a["entities"]["incarnations"]) == 0
    assert b["info"]["started"] == 1 and b["entities"]["incarnations"][69] == 1 and b["rt"]["delay"][69] == sc.IDLE_DELAY
    assert b["echo"] == [[69, sc.payload("Done:1")]]
