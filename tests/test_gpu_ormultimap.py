"""ORMultiMap replicas (AGX_KIND_ORMULTIMAP: ORMap of ORSet) through the HIP engine, against the plain model of
tests/ormultimap_model.py: the reference's known answers (tests/golden/ormultimap_kats.json), crafted two-replica
merges, op edges on 16 replicas and seeded runs, bit-exact on every state word, alive flag and Stats counter -- on
the fused and the multi-pass pipeline.

Every engine gets an explicit msg_capacity: a snapshot row is 20608 B and the row heap holds
2 x (actors rounded to buckets + msg_capacity) of them."""
import json
import pathlib

import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind, Op
from tests import crdt_model as M
from tests import ormultimap_model as P
from tests.crdt_cases import crdt_peer
from tests.test_gpu_parity import COUNT_KEYS

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "ormultimap_kats.json").read_text())["cases"]
W = P.ORMM_WORDS
E = P.ORMultiMap
AGX_ERANGE = 7
CAP = 2048  # msg_capacity of the small engines: a heap of 2 x (32 + 2048) rows, 86 MB
NO_SENDER = 0xFFFFFFFF
U32 = 1 << 32


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as in test_gpu_pncountermap.py)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


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


def run_model(w, drive=None):
    drive = drive or (lambda t: t.run())
    model = P.MmModel(**w.engine_kwargs())
    w.apply_to(model)
    return model, drive(model)


def run_both(w, name, drive=None, check=None, msg_capacity=CAP):
    """The workload through the BSP model and the engine (drive(target) -> stats, default: one run to
    quiescence).  check(model) asserts, before the engine runs, that the case exercises what it is for; then
    every state word, alive flag and counter must agree.  Returns (stats, words, model)."""
    drive = drive or (lambda t: t.run())
    model, so = run_model(w, drive)
    if check:
        check(model)
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), msg_capacity=msg_capacity)))
    try:
        w.apply_to(eng)
        sg = drive(eng)
        words, alive = eng.read_state()
    finally:
        eng.close()
    assert_stats(sg, so, name)
    assert_states(words, alive, model, name)
    return sg, words, model


def workload(name, n, init, dst, pay, throughput=5, fanout=1, seed=1, max_emit=None):
    dst = np.asarray(dst, np.uint32)
    return wl.Workload(f"ormm_{name}", n, W, max_emit or fanout + 1, throughput, 0, [(0, n, Kind.ORMULTIMAP, init)],
                       gossip=(fanout, seed), tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), np.asarray(pay, np.uint32)),
                       bucket_actors=32)


# ------------------------------------------------------------------ 1. the reference's answers
@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_kats_through_the_engine(built, pipeline, case):
    """Each script op by op, one engine run per op; after every op every replica's 2576 words are the model's."""
    eng = GpuEngine(EngineConfig(n_actors=case["replicas"], n_words=W, max_emit=2, bucket_actors=32, msg_capacity=CAP))
    try:
        got = P.run_kat(case, eng)
    finally:
        eng.close()
    want = P.run_kat(case, P.MmModel(case["replicas"], max_emit=2))
    assert len(got) == len(want)
    for i, (g, m) in enumerate(zip(got, want)):
        assert np.array_equal(g, m), f"{case['name']}: after op {i}: engine {[P.from_words(x) for x in g]} model {[P.from_words(x) for x in m]}"


# ------------------------------------------------------------------ 2. crafted two-replica merges
def one_key(node, key, version, vset, vv=None):
    """A replica of `node` that bound `key` once (birth dot node -> version), with the given value set."""
    return E(M.ORSet({key: {node: version}}, vv or {node: version}), {key: vset})


def rand_set(rng, nodes, lo=1, hi=9):
    """A value set over a random non-empty subset of the 8 values with dots of `nodes`; its vvector covers them."""
    el, vv = {}, {}
    for v in range(P.VALUES):
        if v == 0 or rng.random() < 0.6:
            el[v] = {n: int(rng.integers(lo, hi)) for n in nodes if n == nodes[0] or rng.random() < 0.7}
            for n, x in el[v].items():
                vv[n] = max(vv.get(n, 0), x)
    return M.ORSet(el, vv)


def dots_map(total, phase, rng):
    """`total` live key dots in all (1, 2, 3 or 5: the row's dots section is rounded up to 4 u32), on nodes of
    `phase`'s parity, so that two phases are concurrent and keep all their dots."""
    shape = {1: [(10, 1)], 2: [(10, 1), (50, 1)], 3: [(10, 2), (50, 1)], 5: [(10, 2), (20, 2), (63, 1)]}[total]
    dots = {key: {phase + 2 * i: 1 + phase + i for i in range(c)} for key, c in shape}
    vv = {}
    for d in dots.values():
        for n, v in d.items():
            vv[n] = max(vv.get(n, 0), v)
    return E(M.ORSet(dots, vv), {key: rand_set(rng, [phase, phase + 2, phase + 4]) for key in dots})


def full_map(phase):
    """All 64 keys live with 8 key dots each, and in every key all 8 values with 8 dots each; the version vectors
    equal the dots, so two phases are Concurrent and every dot of both sides survives as the larger one."""
    dots = {n: (5 if (n + phase) % 2 == 0 else 3) for n in range(P.NODES)}
    vset = M.ORSet({v: {n: 1 + (n + v + phase) % 4 for n in range(P.NODES)} for v in range(P.VALUES)},
                   {n: 4 for n in range(P.NODES)})
    return E(M.ORSet({k: dict(dots) for k in range(P.ELEMS)}, dots), {k: vset.copy() for k in range(P.ELEMS)})


def versions_pair(base):
    """Two sets whose versions straddle `base`: each side holds the newer dot of half the values, a removal the
    other has not seen, and a removal it has seen."""
    a = M.ORSet({0: {0: base - 1}, 1: {0: base + 1, 1: base}, 2: {1: base - 2}, 5: {0: base}}, {0: base + 1, 1: base})
    b = M.ORSet({0: {0: base - 1}, 1: {1: base + 1}, 3: {1: base + 2}, 5: {0: base}}, {0: base, 1: base + 2})
    return a, b


def merge_cases():
    rng = np.random.default_rng(13)
    out = []
    out.append(("all_64_keys_8_values_8_dots", full_map(0), full_map(1)))
    out.append(("key_0_vs_key_63", one_key(0, 0, 1, rand_set(rng, [0])), one_key(1, 63, 1, rand_set(rng, [1]))))
    out.append(("key_0_both_sides", one_key(0, 0, 2, rand_set(rng, [0, 2])), one_key(1, 0, 1, rand_set(rng, [1, 3]))))
    out.append(("key_63_both_sides", one_key(0, 63, 2, rand_set(rng, [0, 2])), one_key(1, 63, 1, rand_set(rng, [1, 3]))))
    for total in (1, 2, 3, 5):
        out.append((f"live_dots_{total}", dots_map(total, 0, rng), dots_map(total, 1, rng)))
    # a key live on one side only, not dominated: taken over with all 72 u32
    out.append(("one_side_not_dominated", one_key(0, 5, 4, rand_set(rng, [0])), one_key(1, 44, 2, rand_set(rng, [1]))))
    # a key live on one side only whose dots all die in the merge: the other side saw them and removed the key
    seen = E(M.ORSet({44: {1: 2}}, {0: 4, 1: 2}), {44: rand_set(rng, [1])})
    out.append(("key_dots_all_die", one_key(0, 5, 4, rand_set(rng, [0, 1])), seen))
    # a live key with an empty set on one side (put(key, Set())), a bound one on the other
    out.append(("live_key_with_an_empty_set", one_key(0, 7, 2, M.ORSet({}, {0: 3})), one_key(1, 7, 1, rand_set(rng, [0, 1], 1, 6))))
    out.append(("empty_sets_on_both_sides", one_key(0, 7, 2, M.ORSet({}, {0: 3})), one_key(1, 7, 1, M.ORSet({}, {1: 9}))))
    for name, base in (("value_versions_around_2_16", 1 << 16), ("value_versions_around_2_31", 1 << 31)):
        a, b = versions_pair(base)
        out.append((name, one_key(0, 33, 1, a), one_key(1, 33, 1, b)))
    return out


MERGES = merge_cases()


@pytest.mark.parametrize("case", MERGES, ids=[c[0] for c in MERGES])
def test_crafted_merges_both_directions(built, pipeline, case):
    name, a, b = case
    init = np.stack([P.to_words(a), P.to_words(b)])
    if name == "all_64_keys_8_values_8_dots":  # the row fills the whole pitch
        assert all(len(m.values) == 64 and all(len(d) == 8 for d in m.keys.elements.values()) and
                   all(len(s.elements) == 8 and all(len(d) == 8 for d in s.elements.values()) for s in m.values.values()) and
                   P.row_u32(m) == 5152 for m in (a, b))
        assert a.merge(b) != a and a.merge(b) != b
    if name.startswith("live_dots_"):
        assert all(sum(len(d) for d in m.keys.elements.values()) == int(name[10:]) for m in (a, b))
    maps = [a, b]
    for sender in (0, 1):
        w = workload(name, 2, init, [sender], [Op.make(Op.GOSSIP, 0)])
        sg, words, model = run_both(w, f"{name} sender {sender}")
        want = maps[1 - sender].merge(maps[sender])
        assert P.from_words(words[1 - sender]) == want and P.from_words(words[sender]) == maps[sender], name
        assert sg.unhandled == 0 and sg.in_flight == 0
    ab = a.merge(b)
    if name == "one_side_not_dominated":
        assert ab.values == {5: a.values[5], 44: b.values[44]}
    if name == "key_dots_all_die":
        assert ab.values == {44: b.values[44]} and b.merge(a).values == ab.values  # key 5 dropped, its block cleared
        assert not P.to_words(ab).view(np.uint32)[2 * 272 + 72 * 5:2 * 272 + 72 * 6].any()
    if name == "key_0_vs_key_63":
        assert set(ab.values) == {0, 63}
    if name == "live_key_with_an_empty_set":
        assert a.entries == {7: frozenset()} and ab.contains(7)
        assert ab.values[7].elements == {v: d for v, d in ((v, {n: x for n, x in d.items() if not (n == 0 and x <= 3)})
                                                           for v, d in b.values[7].elements.items()) if d}
    if name == "empty_sets_on_both_sides":
        assert ab.entries == {7: frozenset()} and ab.values[7].vvector == {0: 3, 1: 9}
    if name.startswith("value_versions_around"):
        base = 1 << int(name.rsplit("_", 1)[1])
        assert ab.values[33].elements == {0: {0: base - 1}, 1: {0: base + 1, 1: base + 1}, 3: {1: base + 2}, 5: {0: base}}
        assert ab.values[33].vvector == {0: base + 1, 1: base + 2}


# ------------------------------------------------------------------ 3. op edges on 16 replicas
def test_op_edges_and_node_wrap(built, pipeline):
    """put with mask 0 and mask 255, an emptying removeBinding, a removeBinding on an absent key (the version vector
    moves, no key appears), replaceBinding with old == new (nothing at all) and with old != new; replicas 8..15
    write the dots of node id % 8."""
    dst = [3, 3, 9, 1, 12, 12, 15, 15, 6, 6, 6, 10, 10]
    pay = [Op.put_set(7, []), Op.put_set(8, range(8)), Op.add_binding(2, 5), Op.add_binding(2, 5),
           Op.add_binding(63, 0), Op.remove_binding(63, 0), Op.remove_binding(20, 1), Op.make(Op.REMOVE, 21),
           Op.add_binding(0, 4), Op.replace_binding(0, 4, 4), Op.replace_binding(1, 2, 2),
           Op.add_binding(30, 1), Op.replace_binding(30, 1, 6)]
    w = workload("edges", 16, None, dst, pay, throughput=8)
    sg, words, model = run_both(w, "op edges")
    m = [P.from_words(x) for x in words]
    assert m[3].entries == {7: frozenset(), 8: frozenset(range(8))} and m[3].values[7] == M.ORSet()
    assert m[3].values[8].vvector == {3: 8} and m[3].values[8].elements[7] == {3: 8} and m[3].keys.vvector == {3: 2}
    assert m[9].values[2] == M.ORSet({5: {1: 1}}, {1: 1}) and m[9].keys.elements[2] == {1: 1} and m[9] == m[1]  # node wrap
    assert m[12].entries == {} and m[12].keys.vvector == {4: 2} and not words[12, 260:].any()
    assert m[15].entries == {} and m[15].keys.vvector == {7: 1} and not words[15, 260:].any()
    assert m[6] == E().add_binding(6, 0, 4)                                       # both replaces with old == new: untouched
    assert m[10].entries == {30: frozenset({6})} and m[10].keys.elements == {30: {2: 3}} and m[10].values[30].vvector == {2: 2}
    assert sg.unhandled == 0 and sg.delivered == len(dst)


def test_out_of_range_arguments_are_unhandled(built, pipeline):
    bad = [Op.make(Op.ADD, 512), Op.make(Op.ADD, 0xFFFFFF), Op.make(Op.REMOVE_BINDING, 512), Op.make(Op.PUT, 64 * 256),
           Op.make(Op.REPLACE_BINDING, 4096), Op.make(Op.REMOVE, 64), Op.make(Op.INCREMENT, 1), Op.make(Op.DECREMENT, 1),
           Op.make(Op.CLEAR), Op.make(Op.DELTA_TICK, 0), Op.make(11, 1), Op.make(0, 3), Op.make(255, 0)]
    good = [Op.make(Op.ADD, 511), Op.make(Op.PUT, 64 * 256 - 1), Op.make(Op.REPLACE_BINDING, 4095), Op.make(Op.REMOVE_BINDING, 511)]
    w = workload("unhandled", 16, None, [5] * (len(bad) + len(good)), good[:2] + bad + good[2:], throughput=32)
    sg, words, model = run_both(w, "out of range")
    assert sg.unhandled == len(bad) and sg.delivered == len(bad) + len(good) and sg.emitted == 0
    assert P.from_words(words[5]).entries == {63: frozenset(range(7))}


def test_snapshot_sees_the_state_at_its_position(built, pipeline):
    """bind, remove, bind, gossip, bind in one run of one replica (throughput 8): the snapshot row carries the state
    after the third message, the replica ends with the fifth applied."""
    seed = 1
    peer = crdt_peer(seed, 5, 0, 0, 16)
    pay = [Op.add_binding(4, 1), Op.make(Op.REMOVE, 4), Op.add_binding(4, 3), Op.make(Op.GOSSIP, 0), Op.add_binding(4, 2)]
    w = workload("snapshot_position", 16, None, [5] * 5, pay, throughput=8, seed=seed)
    sg, words, model = run_both(w, "snapshot position")
    own, got = P.from_words(words[5]), P.from_words(words[peer])
    assert got.entries == {4: frozenset({3})} and got.keys.elements == {4: {5: 2}} and got.values[4].vvector == {5: 1}
    assert own.entries == {4: frozenset({2, 3})} and own.keys.elements == {4: {5: 3}} and sg.delivered == 6


@pytest.mark.parametrize("poison", [None, "0", "255"])
def test_queued_gossip_is_merged_intact_in_a_later_tick(built, pipeline, monkeypatch, poison):
    """Replica 2 puts two keys and gossips; its peer has eight host binds in front and drains two messages a
    superstep, so the gossip waits in the peer's mailbox and its row is copied forward by its used length
    (bucket_finish) before it is merged -- with the heap poisoned, a row word read and never copied shows."""
    if poison is not None:
        monkeypatch.setenv("AGX_HEAP_POISON", poison)
    seed = 1
    peer = crdt_peer(seed, 2, 0, 0, 16)
    dst = [2, 2, 2] + [peer] * 8
    pay = [Op.put_set(9, range(8)), Op.put_set(40, [1, 6]), Op.make(Op.GOSSIP, 0)] + [Op.add_binding(50 + i, i) for i in range(8)]
    w = workload("queued", 16, None, dst, pay, throughput=2, seed=seed)

    def check(model):
        assert model.queued_gossips == 2 and model.c["supersteps"] == 5

    sg, words, model = run_both(w, "queued gossip", check=check)
    got = P.from_words(words[peer])
    assert got.entries[9] == frozenset(range(8)) and got.entries[40] == frozenset({1, 6}) and len(got.entries) == 10


# a gossip seed for which replica 2's tick goes to PEER and PEER's tick comes back to replica 2
ANOMALY_SEED = next(s for s in range(1, 4000) if crdt_peer(s, crdt_peer(s, 2, 0, 0, 16), 0, 0, 16) == 2)


def test_rebind_after_remove_gets_stale_dots_back_from_a_stale_peer(built, pipeline):
    """Replica 2 binds values 0 and 1 to key 9 and gossips; removes the key and binds value 5, which starts a set
    with a zero version vector; the peer, which still holds the old set, gossips back.  Value 1's old dot returns
    and the new binding, covered by the stale vector, is dropped (tests/test_ormultimap_model.py pins the same on
    the model).  Reproduced, not repaired."""
    peer = crdt_peer(ANOMALY_SEED, 2, 0, 0, 16)
    w = workload("anomaly", 16, None, [2, 2, 2], [Op.add_binding(9, 0), Op.add_binding(9, 1), Op.make(Op.GOSSIP, 0)],
                 throughput=8, seed=ANOMALY_SEED)

    def drive(t):
        t.run()
        t.tell([2, 2], [Op.make(Op.REMOVE, 9), Op.add_binding(9, 5)])
        t.run()
        t.tell([peer], [Op.make(Op.GOSSIP, 0)])
        return t.run()

    sg, words, model = run_both(w, "anomaly", drive)
    got = P.from_words(words[2])
    assert got.keys.elements == {9: {2: 3}} and got.entries == {9: frozenset({1})} and got.values[9] == M.ORSet({1: {2: 2}}, {2: 2})
    assert P.from_words(words[peer]).entries == {9: frozenset({0, 1})}


def test_concurrent_removal_from_a_set_is_lost(built, pipeline):
    """ORMultiMapSpec "not handle concurrent updates to the same set" on 16 replicas: the emptying removeBinding
    drops the key, the peer's concurrent addBinding brings the removed value back."""
    peer = crdt_peer(ANOMALY_SEED, 2, 0, 0, 16)
    w = workload("lost_removal", 16, None, [2, 2], [Op.add_binding(9, 0), Op.make(Op.GOSSIP, 0)], throughput=8, seed=ANOMALY_SEED)

    def drive(t):
        t.run()
        t.tell([2, peer], [Op.remove_binding(9, 0), Op.add_binding(9, 1)])
        t.run()
        t.tell([peer], [Op.make(Op.GOSSIP, 0)])
        return t.run()

    sg, words, model = run_both(w, "lost removal", drive)
    assert P.from_words(words[2]).entries == {9: frozenset({0, 1})}


@pytest.mark.parametrize("what", ["key_set_version", "value_set_version", "value_set_version_put"])
def test_range_errors(built, pipeline, what):
    """A key-set version or a value-set version that would pass 2^32 - 1 (the reference's Long would not wrap)
    raises AGX_ERANGE; a version that reaches 2^32 - 1 exactly does not."""
    if what == "key_set_version":
        init0 = one_key(3, 6, U32 - 2, M.ORSet({0: {3: 5}}, {3: 5}))
        ok, bad = Op.add_binding(7, 1), Op.remove_binding(8, 1)
    elif what == "value_set_version":
        init0 = one_key(3, 6, 9, M.ORSet({0: {3: U32 - 2}}, {3: U32 - 2}))
        ok, bad = Op.add_binding(6, 1), Op.add_binding(6, 2)
    else:
        init0 = one_key(3, 6, 9, M.ORSet({0: {3: U32 - 4}}, {3: U32 - 4}))
        ok, bad = Op.put_set(6, [1, 5, 7]), Op.put_set(6, [2])
    after = P.apply_op(init0, 3, ok)
    assert after.max_version() == U32 - 1
    with pytest.raises(P.VersionRange):
        P.apply_op(after, 3, bad)
    init = np.zeros((16, W), np.uint64)
    init[3] = P.to_words(init0)
    eng = GpuEngine(EngineConfig(n_actors=16, n_words=W, max_emit=2, bucket_actors=32, msg_capacity=CAP))
    try:
        eng.register_range(0, 16, Kind.ORMULTIMAP, init)
        eng.set_gossip(1, 1)
        eng.tell([3], [ok])
        eng.run()
        assert P.from_words(eng.read_state()[0][3]) == after
        eng.tell([3], [bad])
        with pytest.raises(AgxError) as ei:
            eng.run()
        assert ei.value.status == AGX_ERANGE
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. seeded runs against the BSP model
def writers_merge(w):
    """merge_all of the eight writers' maps after their round-0 ops alone."""
    m = P.MmModel(n_actors=w.n_actors)
    m.register_range(0, w.n_actors, Kind.ORMULTIMAP)
    d, _, p = w.tells
    m.tell(d[:160], p[:160])
    m.run()
    return P.merge_all(m.maps[:8])


def census(model):
    """What a seeded case is for: rows stayed queued past a tick, a key was dropped and bound again, a both-sides
    merge changed a set."""
    assert model.queued_gossips > 0, model.queued_gossips
    assert model.key_removals > 0 and model.rebound > 0, (model.key_removals, model.rebound)
    assert model.merge_census.get("both_sides_changed", 0) > 0, model.merge_census


def converged_on(w):
    expected = writers_merge(w)

    def check(model):
        census(model)
        assert model.converged() and all(m == expected for m in model.maps) and len(expected.values) > 3
        assert any(len(s.elements) > 2 for s in expected.values.values())
        assert model.c["in_flight"] == 0 and model.c["unhandled"] == 0
    return check


SEEDED = {
    "throughput_5": (dict(n=24, rounds=10, throughput=5), None),
    "throughput_1_poison_0": (dict(n=20, rounds=16, throughput=1), "0"),
    "throughput_1_poison_255": (dict(n=20, rounds=16, throughput=1), "255"),
    "bounded_mailbox": (dict(n=20, rounds=16, throughput=1, capacity=21), None),
}


@pytest.mark.parametrize("case", list(SEEDED))
def test_seeded_runs_converge_to_the_writers_merge(built, pipeline, monkeypatch, case):
    """A service registry: eight writers collide on a dozen keys and eight values, removes among their bindings;
    every replica gossips to 2 peers a tick.  At throughput 1 gossips wait in the mailboxes for many ticks and their
    rows are copied forward each superstep by their used length; a mailbox of 21 holds a writer's 20 ops and its
    tick and tail-drops gossips behind them."""
    kw, poison = SEEDED[case]
    if poison is not None:
        monkeypatch.setenv("AGX_HEAP_POISON", poison)
    w = wl.crdt_ormultimap(fanout=2, bucket_actors=32, **kw)
    check = converged_on(w)

    def check_case(model):
        check(model)
        if kw["throughput"] == 1:
            assert model.queued_gossips > 300, model.queued_gossips
        if kw.get("capacity"):
            assert model.tail_dropped_gossips > 0 and model.c["dead_letters"] > 0
    sg, words, _ = run_both(w, case, check=check_case)
    assert all(np.array_equal(words[a, :W], words[0, :W]) for a in range(kw["n"]))


def test_three_runs_with_host_writes_between(built, pipeline):
    """Runs that stop on their superstep budget, host binds, unbinds, puts and removes staged in between -- one of
    them removes a key and binds it again while peers still hold its old set."""
    w = wl.crdt_ormultimap(24, rounds=12, fanout=2, bucket_actors=32)

    def drive(t):
        t.run(3)
        t.tell([0, 9, 9, 17, 23], [Op.add_binding(2, 7), Op.remove_binding(2, 7), Op.make(Op.REMOVE, 3),
                                   Op.put_set(50, [0, 3]), Op.replace_binding(2, 1, 4)])
        t.run(4)
        t.tell([8, 0, 0, 19], [Op.add_binding(2, 6), Op.make(Op.REMOVE, 2), Op.add_binding(2, 1), Op.put_set(63, [])])
        t.run(0)  # (a run without mail to drain)
        return t.run()

    def check(model):
        census(model)
        assert model.c["in_flight"] == 0 and model.c["supersteps"] > 7 and len(model.maps[20].values) > 3

    run_both(w, "three runs", drive, check)


def test_hot_bucket_takes_the_skew_launch(built, pipeline):
    """2112 host binds for 16 of the 24 replicas of the one bucket beside the writers' ops and the ticks: the
    bucket's first inbox is more than one tile of 2048 messages, which is what sends a bucket to the skew launch (by
    construction: the model's per-bucket inbox census).  At throughput 30 those replicas drain their 132 ops over
    five supersteps, their ticks behind them and the gossips of the other eight behind those, so rows queue there
    as well."""
    w = wl.crdt_ormultimap(24, rounds=8, fanout=2, throughput=30, bucket_actors=32)
    d, s, p = w.tells
    hot = np.repeat(np.arange(16, dtype=np.uint32), 132)
    j = np.arange(hot.size, dtype=np.uint32)
    ops = np.array([(Op.add_binding if x % 3 else Op.remove_binding)(int(x * 7 % 12), int(x % 8)) for x in j], np.uint32)
    k = 160  # (after the writers' ops, before the ticks)
    w.tells = (np.concatenate([d[:k], hot, d[k:]]), np.concatenate([s[:k], np.full(hot.size, NO_SENDER, np.uint32), s[k:]]),
               np.concatenate([p[:k], ops, p[k:]]))

    def check(model):
        assert model.max_bucket_inbox(32) > 2048, model.max_bucket_inbox(32)
        census(model)
        assert model.c["in_flight"] == 0 and model.c["unhandled"] == 0

    run_both(w, "hot bucket", check=check, msg_capacity=4096)
