"""Children on the GPU (agx_set_children): the HIP engine through the C ABI against the known
answers restated from the reference's specs (tests/golden/children_kats.json) and against the model
(tests/children_model.py, pinned to WatchModel by tests/test_children_model.py), on the fused and the multi-pass
pipelines, with graph replays and eager launches.  Everything is compared bit for bit after every run: states,
alive flags, kinds, every counter, children_info, read_children, watch_info, read_watch, the outbox order, and
conservation."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import NO_SENDER, EngineConfig, GpuEngine, Kind
from tests import children_cases as cc
from tests.children_model import NONE, ChildrenModel

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ECAPACITY, ESTATE = 1, 2, 5, 6
B = typed.Behaviors
ctx = typed.context


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the death-watch fixture)
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
    m = ChildrenModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def status_of(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status


def conserved(st, terminated):
    return st["staged"] + st["emitted"] + terminated == st["delivered"] + st["dead_letters"] + st["in_flight"]


def both(w, script, actors=None):
    """run `script(target)` -- a generator that yields after every run's stats -- on the engine and the model and
    compare everything after every run"""
    eng, mod = engine_for(w), model_for(w)
    actors = range(w.n_actors) if actors is None else actors
    n, sm, m = 0, None, None
    for sg, sm in zip(script(eng), script(mod)):
        sg, sm = cc.counts(sg), cc.counts(sm)
        assert sg == sm, (n, sg, sm)
        g, m = cc.snapshot(eng, actors), cc.snapshot(mod, actors)
        for k in g:
            assert g[k] == m[k], (n, k, g[k], m[k])
        assert np.array_equal(eng.read_kinds(), mod.kind.astype(np.uint8))
        assert conserved(sg, g["watch"]["terminated"])
        n += 1
    eng.close()
    return sm, m


# ------------------------------------------------------------------ 1. the known answers
@pytest.mark.parametrize("T", cc.KAT_T)
@pytest.mark.parametrize("name", cc.KAT_NAMES)
def test_kat(built, pipeline, name, T):
    eng = engine_for(cc.kat_workload(name, T))
    got = cc.run_kat(name, T, eng)
    eng.close()
    print(got)
    cc.check_kat(name, T, got)
    assert got == cc.run_kat(name, T, model_for(cc.kat_workload(name, T)))


# ------------------------------------------------------------------ 2. buckets: same, different, a straddling block
@pytest.mark.parametrize("n,parents,first_child,max_children", [
    (128, (0, 4), 8, 4),      # parents and children in one bucket
    (128, (0, 4), 64, 4),     # in different buckets
    (160, (2, 6), 54, 3),     # children 54..71: the block straddles the bucket boundary at 64; 160 = 5 buckets
    (150, (100, 8), 20, 5),   # parents after their children; the last bucket is partial
])
@pytest.mark.parametrize("T", [1, 3])
def test_shapes(built, pipeline, launch, T, n, parents, first_child, max_children):
    w = cc.parent_workload(T, n=n, parents=parents, first_child=first_child, max_children=max_children)
    p0 = parents[0]
    kid = lambda p, k: first_child + (p - p0) * max_children + k

    def script(t):
        cc.tells(t, *[(p0 + i, "SpawnWatch:%d" % i) for i in range(parents[1])], (p0, "Spawn:9"))
        yield t.run(1)
        cc.tells(t, (kid(p0, 0), "Work:1"), (kid(p0 + 1, 0), "Work:2"), (kid(p0, 1), "Work:3"))
        yield t.run()
        cc.tells(t, (p0, "StopChild"), (p0 + 1, "StopChild"), (p0 + 2, "Stop"), (kid(p0 + 3, 0), "Stop"))
        yield t.run(2)
        yield t.run()
    st, snap = both(w, script)
    ci = snap["children"]
    assert ci["created"] == parents[1] + 1 and ci["child_stops"] == 2 and ci["cascade_stops"] == 1
    assert snap["watch"]["terminated"] == 2  # parent p0 + 1 and p0 + 3 hear of their watched child; p0 stopped its second


# ------------------------------------------------------------------ 3. a tree, grown then stopped at the root
def test_tree_depth_3_fanout_2(built, pipeline, launch):
    depth, fanout = 3, 2
    w = wl.spawn_tree(depth, fanout, throughput=3, bucket_actors=32)
    w.n_actors = 128  # (four buckets; ids 15.. stay unregistered)
    died = {}

    def script(t):
        for st in wl.grow_tree(t, depth, fanout, run=lambda x: x.run()):
            yield st
        t.tell(np.asarray([0], np.uint32), np.asarray([wl.CH_STOP << 24], np.uint32), np.asarray([NO_SENDER], np.uint32))
        for level in range(depth + 1):  # the cascade takes one level per tick
            yield t.run(1)
            _, alive = t.read_state()
            died.setdefault(id(t), []).append(int((alive[:15] & 1).sum()))
        yield t.run()
    st, snap = both(w, script)
    assert all(v == [14, 12, 8, 0] for v in died.values()) and len(died) == 2
    assert sum(snap["alive"]) == 0 and snap["children"]["cascade_stops"] == 14 and snap["children"]["live"] == 0
    assert [k["parent"] for k in snap["kids"][:7]] == [NONE, 0, 0, 1, 1, 2, 2]


# ------------------------------------------------------------------ 4. refused spawns
def test_full_region_and_outsider(built, pipeline):
    w = cc.parent_workload(3, n=128, parents=(0, 2), first_child=40, max_children=2)
    w.ranges = w.ranges + [(10, 1, w.ranges[0][2], None)]  # actor 10: the parent behaviour outside every parent range

    def script(t):
        cc.tells(t, (0, "Spawn"), (0, "Spawn"), (0, "Spawn:7"), (10, "Spawn"))
        yield t.run()
        cc.tells(t, (0, "StopChild"))  # context.stop(0xFFFFFFFF): no child of the actor
        yield t.run()
    st, snap = both(w, script)
    ci = snap["children"]
    assert (ci["spawned"], ci["refused"], ci["created"], ci["illegal_stops"]) == (2, 2, 2, 1)
    assert snap["words"][10][0] == NONE and snap["alive"][0] == 0 and snap["kids"][0]["spawn_count"] == 2
    assert ci["cascade_stops"] == 2  # the actor that stopped by the exception took its two children


# ------------------------------------------------------------------ 5. born and stopped in one tick; tells around the Create
def test_spawn_then_stop_in_one_tick(built, pipeline, launch):
    """throughput 3: Spawn and StopChild are handled in one tick, so the Create and the Stop arrive together: the
    child is born and stopped in that tick, and a Work told in the same tick is a dead letter"""
    w = cc.parent_workload(3, n=128, parents=(0, 4), first_child=64, max_children=4)

    def script(t):
        cc.tells(t, (0, "SpawnWatch"), (0, "StopChild"))
        yield t.run(1)
        cc.tells(t, (64, "Work:5"))
        yield t.run(1)
        yield t.run()
    st, snap = both(w, script)
    ci = snap["children"]
    assert (ci["created"], ci["child_stops"], ci["live"]) == (1, 1, 0) and snap["alive"][64] == 0
    assert st["dead_letters"] == 1 and snap["watch"]["terminated"] == 1 and snap["kids"][64]["created"] == 1


def test_tell_before_and_with_the_create(built, pipeline):
    """a tell that reaches the child id one tick before its Create is a dead letter; one in the Create's tick is
    delivered, wherever the Create stands in the inbox"""
    w = cc.parent_workload(1, n=128, parents=(0, 4), first_child=64, max_children=4)

    def script(t):
        cc.tells(t, (0, "Spawn"), (64, "Work:1"))   # tick 1: the spawn; the Work is early
        yield t.run(1)
        cc.tells(t, (64, "Work:2"))                 # tick 2: [Create from tick 1, Work] -- the Create is emitted mail, the Work staged
        yield t.run(1)
        yield t.run()
    st, snap = both(w, script)
    assert snap["words"][64] == [1, 0] and st["dead_letters"] == 1


def test_create_takes_no_mailbox_room(built, pipeline):
    """the child's bounded mailbox has capacity 1: the Create takes no room, the Work of the same tick is admitted"""
    w = cc.parent_workload(3, n=128, parents=(0, 4), first_child=64, max_children=4)
    w.mailbox_classes = {1: 1}
    w.mailboxes = [(64, 16, 1)]

    def script(t):
        cc.tells(t, (0, "Spawn"))
        yield t.run(1)
        cc.tells(t, (64, "Work:1"), (64, "Work:2"))  # tick 2: Create, Work, Work: one Work admitted, one dropped
        yield t.run()
    st, snap = both(w, script)
    assert snap["words"][64][0] == 1 and st["dead_letters"] == 1 and snap["children"]["created"] == 1


# ------------------------------------------------------------------ 6. the setup block
def test_spawn_children_before_and_between_runs(built, pipeline, launch):
    w = cc.parent_workload(3, n=128, parents=(0, 8), first_child=60, max_children=3)
    w.children = dict(w.children, spawns=[(0, 8, 0, 5)])

    def script(t):
        yield t.run()                      # the Creates arrive in tick 1
        cc.tells(t, (3, "Stop"))
        yield t.run()
        t.spawn_children(2, 4, 0, 6)       # actor 3 is stopped: skipped
        t.spawn_children(0, 8, 0, 7)
        t.spawn_children(2, 1, 0, 8)       # actor 2's block is full: refused
        yield t.run()
    st, snap = both(w, script)
    ci = snap["children"]
    assert (ci["spawned"], ci["refused"], ci["created"], ci["cascade_stops"]) == (8 + 3 + 7, 1, 18, 1)
    assert snap["words"][60] == [5, 0] and snap["kids"][2]["spawn_count"] == 3 and snap["kids"][3]["spawn_count"] == 1


def test_quiescence(built, pipeline, launch):
    """agx_run(n) lets exactly the model's number of ticks pass: a parent's stop keeps the engine active while a
    created child is alive, and budgets that end inside the cascade"""
    w = cc.parent_workload(3, n=128, parents=(0, 4), first_child=64, max_children=4)
    ticks = []

    def script(t):
        cc.tells(t, (0, "Spawn"), (0, "Spawn"))
        yield t.run()
        cc.tells(t, (0, "Stop"))
        for budget in (1, 1, 1 << 30, 1 << 30):
            st = t.run(budget)
            ticks.append(t.watch_info()["ticks"])
            yield st
    st, snap = both(w, script)
    assert ticks[0::2] == ticks[1::2] and ticks[0::2] == [3, 4, 4, 4]
    assert snap["children"]["cascade_stops"] == 2


# ------------------------------------------------------------------ 7. pool router, larger than the watch slots
def test_pool_router(built, pipeline):
    w = wl.pool_router(6, 6, throughput=3, bucket_actors=32, host_id=128)
    w.n_actors = 128

    def script(t):
        yield t.run()
        d = np.repeat(np.arange(6, dtype=np.uint32), 7)
        t.tell(d, (wl.CH_WORK << 24) | np.arange(d.size, dtype=np.uint32), np.full(d.size, NO_SENDER, np.uint32))
        yield t.run()
        kids = np.arange(6, 6 + 36, dtype=np.uint32)
        t.tell(kids[kids != 8], np.uint32(wl.CH_STOP << 24), np.full(35, NO_SENDER, np.uint32))  # routee 2 of router 0 lives
        yield t.run()
    st, snap = both(w, script)
    assert snap["alive"][:6] == [1, 0, 0, 0, 0, 0] and snap["alive"][8] == 1 and snap["children"]["live"] == 1
    assert snap["words"][6][0] == 2 and snap["words"][11][0] == 1  # seven messages round-robin over six routees


# ------------------------------------------------------------------ 8. the refusals, each with its status
def plain_engine(watch=True, **cfg):
    eng = GpuEngine(EngineConfig(**dict(dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1), **cfg)))
    eng.register_range(0, 32, Kind.COUNTER)
    if watch:
        eng.set_death_watch(2)
    return eng


SITE = [(typed.KIND_COMPILED, 0, None)]


def test_refuses_without_death_watch_either_order(built):
    eng = plain_engine(watch=False)
    assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], SITE)) == EINVAL
    eng.set_death_watch(2)
    eng.set_children([(0, 4, 40, 2)], SITE)
    assert status_of(lambda: eng.set_death_watch(3)) == EINVAL  # (the slot count is fixed once children are set)
    eng.close()
    eng = plain_engine(watch=False)
    assert status_of(lambda: eng.spawn_children(0, 1, 0, 0)) == EINVAL
    eng.tell(0, 1)
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


def test_refuses_after_the_first_run(built):
    eng = plain_engine()
    eng.tell(0, 1)
    eng.run()
    assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], SITE)) == ESTATE
    eng.close()


@pytest.mark.parametrize("regions", [
    [(0, 4, 40, 2), (2, 4, 50, 2)],        # parent ranges overlap
    [(0, 4, 40, 2), (8, 4, 44, 2)],        # child blocks overlap
    [(0, 4, 2, 2)],                        # the child block inside its own parent range
    [(0, 4, 60, 2)],                       # the child block leaves [0, n_actors)
    [(0, 0, 40, 2)], [(0, 4, 40, 0)],      # empty
    [(0, 4, 30, 2)],                       # registered ids (30, 31) in the child block
    [(i, 1, 40 + i, 1) for i in range(9)]  # nine regions
])
def test_refuses_bad_regions(built, regions):
    eng = plain_engine()
    assert status_of(lambda: eng.set_children(regions, SITE)) == EINVAL
    eng.close()


def test_refuses_bad_sites_and_register_range(built):
    eng = plain_engine()
    assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], [(Kind.COUNTER, 0, None)])) == EINVAL
    assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], SITE * 65)) == EINVAL
    eng.set_children([(0, 4, 40, 2), (40, 8, 48, 2)], SITE)   # (grandchildren: a child block inside a parent range)
    assert status_of(lambda: eng.register_range(47, 2, Kind.COUNTER)) == EINVAL
    assert status_of(lambda: eng.register_range(0, 64, Kind.COUNTER)) == EINVAL
    eng.register_range(32, 8, Kind.COUNTER)
    assert status_of(lambda: eng.spawn_children(0, 4, 1, 0)) == EINVAL       # no such site
    assert status_of(lambda: eng.spawn_children(0, 4, 0, 1 << 18)) == EINVAL  # the argument has 18 bits
    eng.tell(0, 1)
    assert status_of(lambda: eng.run()) == EINVAL   # the site's kind is no behaviour of the (missing) tables
    eng.close()


def test_refuses_reserved_tags(built):
    """agx_stage_tells (eng.tell) and agx_tell (eng.tell_one) refuse the Create and Stop tags; tables that name them
    are refused in either call order"""
    eng = plain_engine()
    eng.set_children([(0, 4, 40, 2)], SITE)
    for tag in (0xFD, 0xFC):
        assert status_of(lambda: eng.tell(0, tag << 24 | 1)) == EINVAL
        assert status_of(lambda: eng.tell_one(0, tag << 24 | 1)) == EINVAL
    eng.close()
    st = typed.State("a", "b")
    sends = typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [typed.self_ref(1).tell(0, tag=0xFD), B.same]).build("s")
    tests_ = typed.ReceiveBuilder.create(st).on_message(typed.MessageType("X", 0xFC), lambda m, s: [s.a.inc(), B.same]).build("t")
    for b in (sends, tests_):
        tb = typed.compile_behaviors([b], max_emit=1)
        eng = plain_engine()
        eng.set_children([(0, 4, 40, 2)], SITE)
        assert status_of(lambda: eng.set_behaviors(tb)) == EINVAL
        eng.close()
        eng = plain_engine()
        eng.set_behaviors(tb)
        assert status_of(lambda: eng.set_children([(0, 4, 40, 2)], SITE)) == EINVAL
        eng.close()
    eng = plain_engine()   # without children the tags are ordinary ones
    eng.tell(0, 0xFD000001)
    assert eng.run().delivered == 1
    eng.close()


def test_refuses_two_emitting_actions(built):
    """typed.py refuses such a case; hand-made tables reach agx_set_behaviors"""
    cases = (typed.AgxCase * 1)(typed.AgxCase(result=typed.RES_SAME, act_first=0, act_count=2))
    acts = (typed.AgxAct * 2)(typed.AgxAct(op=typed.A_SPAWN, dword=0), typed.AgxAct(op=typed.A_TELL, dsrc=typed.V_SELF, dk=1))
    tb = typed.Tables([None], cases, acts, np.asarray([0, 1], np.uint32), 2)
    eng = plain_engine()
    assert status_of(lambda: eng.set_behaviors(tb)) == EINVAL
    eng.close()


def test_child_tables_without_children(built):
    w = cc.parent_workload(3)
    w.children = {}
    eng = engine_for(w)
    cc.tells(eng, (0, "Spawn"))
    assert status_of(lambda: eng.run()) == EINVAL
    eng.close()


def test_over_one_tile(built, pipeline):
    """a bucket over one 2048-message tile is AGX_ECAPACITY, sticky, as on every engine with death watch"""
    w = cc.parent_workload(3, n=128, parents=(0, 4), first_child=64, max_children=4)
    eng = engine_for(w)
    eng.tell(np.full(2049, 1, np.uint32), np.arange(2049, dtype=np.uint32) | (cc.TAGS["Work"] << 24), np.full(2049, NO_SENDER, np.uint32))
    assert status_of(lambda: eng.run(1)) == ECAPACITY
    assert status_of(lambda: eng.run(1)) == ECAPACITY
    eng.close()


# ------------------------------------------------------------------ 9. children set, none spawned: the death-watch engine
def test_unused_children_equal_death_watch(built, pipeline):
    from tests import watch_cases as wc
    from tests.watch_model import WatchModel
    n = 96
    w = wc.mix_workload(n + 4, 3)
    w.ranges = [(0, n, w.ranges[0][2], None)]
    w.outbound = (n + 4, 1)
    eng = engine_for(w)
    eng.set_children([(0, 2, n, 2)], [])
    mod = WatchModel(**w.engine_kwargs())
    w.apply_to(mod)
    for dst, pay in wc.mix_rounds(n, 3):
        for t in (eng, mod):
            t.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
        assert wc.counts(eng.run(3)) == wc.counts(mod.run(3))
        g, m = wc.snapshot(eng, range(n)), wc.snapshot(mod, range(n))
        for k in g:
            assert g[k] == m[k], k
    assert eng.children_info() == dict.fromkeys(cc.CHILD_KEYS, 0)
    eng.close()
