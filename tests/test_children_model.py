"""The model of DESIGN.md §2.6 (tests/children_model.py) on the CPU: with no region set, and with regions set but
no spawn, it is WatchModel (itself pinned to the frozen oracle) bit for bit on watch_cases.mix_workload; and it
gives the known answers restated from the reference's specs (tests/golden/children_kats.json)."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER
from tests import children_cases as cc
from tests import watch_cases as wc
from tests.children_model import NONE, ChildrenModel
from tests.watch_model import WatchModel


def model_for(w, cls=ChildrenModel):
    m = cls(**w.engine_kwargs())
    w.apply_to(m)
    return m


def run_mix(m, n, seed):
    out = []
    for dst, pay in wc.mix_rounds(n, seed):
        m.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
        st = wc.counts(m.run(3))
        out.append((st, wc.snapshot(m, range(n))))
    out.append((wc.counts(m.run()), wc.snapshot(m, range(n))))
    return out, m.kind.copy(), m.died[:], m.now


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("T", [1, 3])
def test_equals_watch_model(T, seed):
    """no region set: WatchModel bit for bit"""
    n = 96
    ref = run_mix(model_for(wc.mix_workload(n, T), WatchModel), n, seed)
    got = run_mix(model_for(wc.mix_workload(n, T)), n, seed)
    assert repr(got) == repr(ref)


@pytest.mark.parametrize("T", [1, 3])
def test_regions_without_spawn_equal_watch_model(T):
    """regions set, nothing spawned: the registered actors behave as in WatchModel; the child block (ids 96..99,
    unregistered) differs only in its death ticks: "none" instead of "dead before tick 1" """
    n = 96
    def build(cls):
        w = wc.mix_workload(n + 4, T)
        w.ranges = [(0, n, w.ranges[0][2], None)]
        w.outbound = (n + 4, 1)
        m = model_for(w, cls)
        return m
    a, b = build(WatchModel), build(ChildrenModel)
    b.set_children([(0, 2, n, 2)], [])
    for dst, pay in wc.mix_rounds(n, 7):
        for m in (a, b):
            m.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))
        sa, sb = wc.counts(a.run(3)), wc.counts(b.run(3))
        assert sa == sb
        assert repr(wc.snapshot(a, range(n))) == repr(wc.snapshot(b, range(n)))
    assert wc.counts(a.run()) == wc.counts(b.run())
    assert np.array_equal(a.kind, b.kind) and a.now == b.now
    assert a.died[:n] == b.died[:n] and all(x == NONE for x in b.died[n:]) and all(x == 0 for x in a.died[n:])
    assert b.children_info() == dict.fromkeys(cc.CHILD_KEYS, 0)


@pytest.mark.parametrize("T", cc.KAT_T)
@pytest.mark.parametrize("name", cc.KAT_NAMES)
def test_kat(name, T):
    got = cc.run_kat(name, T, model_for(cc.kat_workload(name, T)))
    print(got)
    cc.check_kat(name, T, got)


def test_tree_grows_and_dies_one_level_per_tick():
    depth, fanout = 3, 2
    w = wl.spawn_tree(depth, fanout, throughput=3, bucket_actors=32)
    m = model_for(w)
    wl.grow_tree(m, depth, fanout)
    _, alive = m.read_state()
    assert alive.sum() == w.n_actors == 15 and m.children_info()["live"] == 14
    m.tell(np.asarray([0], np.uint32), np.asarray([wl.CH_STOP << 24], np.uint32))
    t0 = m.now
    m.run()
    _, alive = m.read_state()
    assert alive.sum() == 0 and m.children_info()["cascade_stops"] == 14
    assert [m.died[a] - t0 for a in (0, 1, 3, 7)] == [1, 2, 3, 4]  # one level per tick
    for first, count in wl.spawn_tree_levels(depth, fanout)[1:]:
        for a in range(first, first + count):
            assert m.read_children(a)["parent"] == (a - 1) // 2 and m.words[a, 1] == (a - 1) // 2


def test_full_region_and_outsider():
    w = cc.parent_workload(3, parents=(0, 2), first_child=40, max_children=2)
    w.ranges = w.ranges + [(10, 1, w.ranges[0][2], None)]  # actor 10 runs the parent behaviour outside every parent range
    m = model_for(w)
    cc.tells(m, (0, "Spawn"), (0, "Spawn"), (0, "Spawn:7"), (10, "Spawn"))
    m.run()
    info = m.children_info()
    assert (info["spawned"], info["refused"], info["created"]) == (2, 2, 2)
    assert m.words[0, 0] == NONE and m.words[10, 0] == NONE and m.read_children(0)["spawn_count"] == 2
