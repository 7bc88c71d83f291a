"""LWWMap replicas (AGX_KIND_LWWMAP: ORMap of LWWRegister) through the HIP engine, against the plain
model of tests/lwwmap_model.py: the reference's known answers (tests/golden/lwwmap_kats.json), crafted
two-replica merges, and seeded runs bit-exact on every state word, alive flag and Stats counter -- on
the fused and the multi-pass pipeline."""
import json
import pathlib

import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind, Op
from tests import crdt_model as M
from tests import lwwmap_model as L
from tests.test_gpu_parity import COUNT_KEYS

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "lwwmap_kats.json").read_text())["cases"]
W = L.LWWMAP_WORDS
AGX_ERANGE = 7


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as in test_gpu_crdt_states.py)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


def engine_for(w, **cfg):
    return GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), **cfg)))


def assert_states(words, alive, model, name):
    mw, ma = model.read_state()
    assert np.array_equal(alive, ma), f"{name}: alive differs"
    diff = np.nonzero((words[:, :W] != mw[:, :W]).any(axis=1))[0]
    if diff.size:
        r = int(diff[0])
        cols = np.nonzero(words[r, :W] != mw[r, :W])[0]
        raise AssertionError(f"{name}: {diff.size} replicas differ, first {r} at words {cols[:8]}: "
                             f"engine {words[r, cols[:8]]} model {mw[r, cols[:8]]}")


def assert_stats(sg, so, name):
    for k in COUNT_KEYS:
        assert getattr(sg, k) == so[k], f"{name}: {k} gpu={getattr(sg, k)} model={so[k]}"
    assert sg.staged + sg.emitted == sg.delivered + sg.dead_letters + sg.in_flight, name


def run_both(w, name, drive=None, **cfg):
    """The workload through the engine and the BSP model (drive(target) -> stats, default: one run to
    quiescence); every state word, alive flag and counter must agree.  Returns (stats, words, model)."""
    drive = drive or (lambda t: t.run())
    eng = engine_for(w, **cfg)
    try:
        w.apply_to(eng)
        sg = drive(eng)
        words, alive = eng.read_state()
    finally:
        eng.close()
    model = L.LwwModel(**w.engine_kwargs())
    w.apply_to(model)
    so = drive(model)
    assert_stats(sg, so, name)
    assert_states(words, alive, model, name)
    return sg, words, model


# ------------------------------------------------------------------ 1. the reference's answers
@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_kats_through_the_engine(built, pipeline, case):
    """Each script op by op, one engine run per op; after every op every replica's 356 words are the model's."""
    eng = GpuEngine(EngineConfig(n_actors=case["replicas"], n_words=W, max_emit=2, bucket_actors=32))
    try:
        got = L.run_kat(case, eng)
    finally:
        eng.close()
    want = L.run_kat(case, L.LwwModel(case["replicas"], max_emit=2))
    assert len(got) == len(want)
    for i, (g, m) in enumerate(zip(got, want)):
        assert np.array_equal(g, m), f"{case['name']}: after op {i}: engine {[L.from_words(x) for x in g]} model {[L.from_words(x) for x in m]}"


# ------------------------------------------------------------------ 2. crafted two-replica merges
def one_key(node, key, version, value, ts, vv=None):
    """A replica of `node` that put `key` once (birth dot node -> version)."""
    return L.LWWMap(M.ORSet({key: {node: version}}, vv or {node: version}), {key: (node, value, ts)})


def full_map(phase, rng):
    """All 64 keys live with 8 dots each; the version vector equals the dots, so two phases are Concurrent
    and every dot of both sides survives as the larger one."""
    dots = {n: (5 if (n + phase) % 2 == 0 else 3) for n in range(L.NODES)}
    values = {k: (int(rng.integers(0, 8)), int(rng.integers(0, 1 << 18)), int(rng.integers(-(1 << 62), 1 << 62)))
              for k in range(L.ELEMS)}
    return L.LWWMap(M.ORSet({k: dict(dots) for k in range(L.ELEMS)}, dots), values)


def merge_cases():
    big = [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**62, L.INT64_MAX - 1, L.INT64_MAX]
    out = [("equal_ts_lower_node_wins", "default", one_key(0, 9, 1, 100, 77), one_key(1, 9, 1, 200, 77))]
    for i, t in enumerate(big[:-1]):  # neighbours across every boundary, the larger on either side
        out.append((f"ts_{t}_vs_{big[i + 1]}", "default", one_key(0, 3, 1, 11, t), one_key(1, 3, 1, 22, big[i + 1])))
        out.append((f"ts_{big[i + 1]}_vs_{t}", "default", one_key(0, 60, 1, 11, big[i + 1]), one_key(1, 60, 1, 22, t)))
    out.append(("hi_word_decides", "default", one_key(0, 3, 1, 11, (5 << 32) | 1), one_key(1, 3, 1, 22, (4 << 32) | 0xFFFFFFF0)))
    out.append(("negative_ts_reverse", "reverse", one_key(0, 7, 1, 11, -5), one_key(1, 7, 1, 22, -(2**32) - 1)))
    out.append(("negative_vs_positive", "reverse", one_key(0, 7, 1, 11, -1), one_key(1, 7, 1, 22, 1)))
    out.append(("int64_min_vs_neighbour", "reverse", one_key(0, 7, 1, 11, L.INT64_MIN), one_key(1, 7, 1, 22, L.INT64_MIN + 1)))
    # a key live on one side only, not dominated: taken over with its register
    out.append(("one_side_not_dominated", "default", one_key(0, 5, 4, 11, 40), one_key(1, 44, 2, 22, 2**40)))
    # a key live on one side only and dominated by the other's version vector: dropped, register zeroed
    seen = L.LWWMap(M.ORSet({44: {1: 2}}, {0: 4, 1: 2}), {44: (1, 22, 9)})
    out.append(("one_side_dominated", "default", one_key(0, 5, 4, 11, 40), seen))
    rng = np.random.default_rng(5)
    out.append(("all_64_keys_8_dots", "default", full_map(0, rng), full_map(1, rng)))
    return out


MERGES = merge_cases()


@pytest.mark.parametrize("case", MERGES, ids=[c[0] for c in MERGES])
def test_crafted_merges_both_directions(built, pipeline, case):
    name, clock, a, b = case
    init = np.stack([L.to_words(a), L.to_words(b)])
    if name == "all_64_keys_8_dots":
        assert all(len(m.keys.elements) == 64 and all(len(d) == 8 for d in m.keys.elements.values()) for m in (a, b))
    for sender in (0, 1):
        w = wl.Workload(f"lww_{name}", 2, W, 2, 5, 0, [(0, 2, Kind.LWWMAP, init)], gossip=(1, 1), lwwmap=(clock, 0),
                        tells=(np.array([sender], np.uint32), np.array([0xFFFFFFFF], np.uint32),
                               np.array([Op.make(Op.GOSSIP, 0)], np.uint32)), bucket_actors=32)
        sg, words, model = run_both(w, f"{name} sender {sender}")
        maps = [a, b]
        want = maps[1 - sender].merge(maps[sender])
        assert L.from_words(words[1 - sender]) == want and L.from_words(words[sender]) == maps[sender], name
        assert sg.unhandled == 0 and sg.in_flight == 0
    if name == "equal_ts_lower_node_wins":
        assert want.values[9][:2] == (0, 100)
    if name == "one_side_dominated":
        assert a.merge(b).entries == {44: 22} and b.merge(a).entries == {44: 22}  # key 5 dropped, its register zeroed


@pytest.mark.parametrize("clock", ["default", "reverse"])
def test_put_after_remove_restarts_the_clock(built, pipeline, clock):
    """LWWMap.put on an absent key builds a fresh register: clock(0), not clock(the removed timestamp)."""
    far = 10**12 if clock == "default" else -(10**12)
    init = np.stack([L.to_words(one_key(0, 6, 1, 5, far)), L.to_words(L.LWWMap())])
    tells = ([0, 0, 0], [Op.make(Op.REMOVE, 6), Op.put(6, 8), Op.put(63, 9)])
    w = wl.Workload("lww_restart", 2, W, 2, 5, 0, [(0, 2, Kind.LWWMAP, init)], gossip=(1, 1), lwwmap=(clock, 1000),
                    tells=(np.array(tells[0], np.uint32), np.full(3, 0xFFFFFFFF, np.uint32), np.array(tells[1], np.uint32)),
                    bucket_actors=32)
    _, words, _ = run_both(w, f"restart {clock}")
    m = L.from_words(words[0])
    assert m.values[6] == (0, 8, 1001 if clock == "default" else -1001) and m.keys.elements[6] == {0: 2}


def test_put_at_int64_max_is_a_range_error(built, pipeline):
    init = np.stack([L.to_words(one_key(0, 6, 1, 5, L.INT64_MAX)), L.to_words(L.LWWMap())])
    eng = GpuEngine(EngineConfig(n_actors=2, n_words=W, max_emit=2, bucket_actors=32))
    try:
        eng.register_range(0, 2, Kind.LWWMAP, init)
        eng.set_gossip(1, 1)
        eng.tell([0], [Op.put(6, 1)])
        with pytest.raises(AgxError) as ei:
            eng.run()
        assert ei.value.status == AGX_ERANGE
    finally:
        eng.close()
    with pytest.raises(L.TimestampRange):
        one_key(0, 6, 1, 5, L.INT64_MAX).put(0, 6, 1, L.default_clock, 1)


# ------------------------------------------------------------------ 3 / 4. seeded runs against the BSP model
@pytest.mark.parametrize("n", [9, 16])
def test_node_wrap(built, pipeline, n):
    """Replica 8 shares node 0 with replica 0: both write node 0's dots and registers."""
    w = wl.crdt_lwwmap(n, rounds=6, fanout=2, bucket_actors=32)
    d, s, p = w.tells
    extra = np.array([Op.put(1, 77), Op.put(40, 78), Op.make(Op.REMOVE, 1), Op.put(1, 79)], np.uint32)
    k = 8 * 20  # (after the writers' ops, before the ticks: replica 8 writes as node 0 too)
    w.tells = (np.concatenate([d[:k], np.full(4, 8, np.uint32), d[k:]]), np.concatenate([s[:k], s[:4], s[k:]]),
               np.concatenate([p[:k], extra, p[k:]]))
    _, words, model = run_both(w, f"node wrap {n}")
    assert model.maps[8].keys.vvector.get(0, 0) > 0 and model.c["unhandled"] == 0


def test_three_buckets_cross_bucket_gossip(built, pipeline):
    sg, _, model = run_both(wl.crdt_lwwmap(96, rounds=8, bucket_actors=32), "96 replicas, buckets of 32")
    assert sg.in_flight == 0 and len(model.maps[95].values) > 3


def test_default_buckets_second_partly_filled(built, pipeline):
    sg, _, model = run_both(wl.crdt_lwwmap(600, rounds=5), "600 replicas, buckets of 512")
    assert sg.in_flight == 0


@pytest.mark.parametrize("poison", ["0", "255"])
def test_queued_gossips_rows_copied_forward(built, pipeline, monkeypatch, poison):
    """throughput 1, fanout 3: gossips wait in the mailboxes for several ticks, their rows are copied forward
    each superstep by their used length; with the heap poisoned, a row word read and never written shows."""
    monkeypatch.setenv("AGX_HEAP_POISON", poison)
    w = wl.crdt_lwwmap(48, rounds=5, fanout=3, throughput=1, bucket_actors=32)
    sg, _, model = run_both(w, f"queued rows poison {poison}")
    assert model.queued_gossips > 200, model.queued_gossips  # (the census: rows did queue)
    assert sg.in_flight == 0


def test_bounded_mailbox_tail_drops_gossips(built, pipeline):
    w = wl.crdt_lwwmap(64, rounds=6, fanout=3, throughput=1, capacity=2, bucket_actors=32)
    sg, _, model = run_both(w, "capacity 2")
    assert model.tail_dropped_gossips > 0 and model.queued_gossips > 0 and sg.dead_letters > 0


@pytest.mark.parametrize("clock", ["default", "reverse"])
def test_three_runs_with_host_writes_between(built, pipeline, clock):
    """Runs that stop on their superstep budget, host puts and removes staged in between: the timestamps come
    from later steps, with the base far from 0."""
    base = 1_700_000_000_000
    w = wl.crdt_lwwmap(40, rounds=14, fanout=2, bucket_actors=32, clock=clock, base=base)

    def drive(t):
        t.run(3)
        t.tell([0, 9, 9, 17, 39], [Op.put(2, 500), Op.put(2, 501), Op.make(Op.REMOVE, 3), Op.put(50, 502), Op.put(2, 503)])
        t.run(4)
        t.tell([8, 0, 33], [Op.put(2, 600), Op.make(Op.REMOVE, 2), Op.put(63, 601)])
        t.run(0)  # (a run without mail to drain: no superstep, the clock stands)
        return t.run()

    sg, words, model = run_both(w, f"three runs {clock}", drive)
    ts = [r[2] for m in model.maps for r in m.values.values()]
    assert sg.in_flight == 0 and (max(ts) > base + 7 if clock == "default" else min(ts) < -base - 7)
    assert all((t > base) if clock == "default" else (t < -base) for t in ts)


def test_hot_buckets_take_the_skew_launch(built, pipeline):
    """Every replica gossips to 70 peers a tick, so each bucket of 32 receives about 2240 messages a superstep:
    more than one tile of 2048, which is what sends a bucket to the skew launch (by construction: the model's
    per-bucket inbox census).  The merges, the snapshot rows and the queued rows' copies all run there."""
    w = wl.crdt_lwwmap(96, rounds=3, fanout=70, throughput=40, bucket_actors=32)
    sg, _, model = run_both(w, "skew", msg_capacity=1 << 15)
    assert model.max_bucket_inbox(32) > 2048, model.max_bucket_inbox(32)
    assert model.queued_gossips > 0 and sg.in_flight == 0


def test_host_puts_behind_a_hot_bucket_backlog(built, pipeline):
    """The same load with host puts staged after two ticks: they queue behind backlogs of more than one drain
    and are drained supersteps later, inside replays whose buckets take the skew launch (on the fused
    pipeline a strict replay defers such a bucket and the host re-runs that superstep): each put's timestamp
    must still be the number of the superstep that drained it."""
    base = 5_000_000
    w = wl.crdt_lwwmap(96, rounds=4, fanout=70, throughput=40, bucket_actors=32, base=base)

    def drive(t):
        t.run(2)
        t.tell([3, 40, 40, 77, 95], [Op.put(50, 1), Op.put(51, 2), Op.put(50, 3), Op.make(Op.REMOVE, 0), Op.put(52, 4)])
        return t.run()

    sg, _, model = run_both(w, "skew with host puts", drive, msg_capacity=1 << 15)
    assert model.max_bucket_inbox(32) > 2048 and sg.in_flight == 0
    ts = {k: max(m.values[k][2] for m in model.maps if k in m.values) for k in (50, 51, 52)}
    assert all(t > base + 3 for t in ts.values()), ts  # (staged before superstep 3, drained later than that)


# ------------------------------------------------------------------ 5. convergence
def test_convergence_to_the_writers_merge(built, pipeline):
    """A write phase, then gossip only, until the model says every replica is equal: the engine's replicas are
    then equal to each other and to merge_all of the writers (the writers apply all their ops before their
    first tick and before any merge, so no remove is concurrent with another node's put: the merge is a join)."""
    n, fanout = 64, 2
    probe = wl.crdt_lwwmap(n, rounds=1, fanout=fanout, bucket_actors=32)
    ops_only = L.LwwModel(**probe.engine_kwargs())
    ops_only.register_range(0, n, Kind.LWWMAP)
    d, s, p = probe.tells
    ops_only.tell(d[:160], p[:160])
    ops_only.run()
    expected = L.merge_all(ops_only.maps[:8])
    rounds = None
    for r in range(2, 40):  # the number of rounds comes from the model
        m = L.LwwModel(**probe.engine_kwargs())
        wl.crdt_lwwmap(n, rounds=r, fanout=fanout, bucket_actors=32).apply_to(m)
        m.run()
        if m.converged():
            rounds = r
            break
    assert rounds is not None
    _, words, model = run_both(wl.crdt_lwwmap(n, rounds=rounds, fanout=fanout, bucket_actors=32), f"convergence in {rounds}")
    assert all(np.array_equal(words[a, :W], words[0, :W]) for a in range(n))
    got = L.from_words(words[0])
    assert got.entries == expected.entries and got.values == expected.values and got.keys == expected.keys
    assert len(got.values) > 3
