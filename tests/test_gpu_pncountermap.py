"""PNCounterMap replicas (AGX_KIND_PNCOUNTERMAP: ORMap of PNCounter) through the HIP engine, against the
plain model of tests/pncountermap_model.py: the reference's known answers
(tests/golden/pncountermap_kats.json), crafted two-replica merges, ops on 16 replicas and seeded runs,
bit-exact on every state word, alive flag and Stats counter -- on the fused and the multi-pass pipeline.

Every engine gets an explicit msg_capacity: a snapshot row is 10368 B and the row heap holds
2 x (actors rounded to buckets + msg_capacity) of them."""
import json
import pathlib

import numpy as np
import pytest

from akka_amd import workloads as wl
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind, Op
from tests import crdt_model as M
from tests import pncountermap_model as P
from tests.crdt_cases import crdt_peer
from tests.test_gpu_parity import COUNT_KEYS

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "pncountermap_kats.json").read_text())["cases"]
W = P.PNCMAP_WORDS
AGX_ERANGE = 7
CAP = 2048  # msg_capacity of the small engines: a heap of 2 x (32 .. 64 + 2048) rows, 43-44 MB
NO_SENDER = 0xFFFFFFFF


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as in test_gpu_lwwmap.py)
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
    model = P.PncModel(**w.engine_kwargs())
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
    return wl.Workload(f"pnc_{name}", n, W, max_emit or fanout + 1, throughput, 0, [(0, n, Kind.PNCOUNTERMAP, init)],
                       gossip=(fanout, seed), tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), np.asarray(pay, np.uint32)),
                       bucket_actors=32)


# ------------------------------------------------------------------ 1. the reference's answers
@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_kats_through_the_engine(built, pipeline, case):
    """Each script op by op, one engine run per op; after every op every replica's 1296 words are the model's."""
    eng = GpuEngine(EngineConfig(n_actors=case["replicas"], n_words=W, max_emit=2, bucket_actors=32, msg_capacity=CAP))
    try:
        got = P.run_kat(case, eng)
    finally:
        eng.close()
    want = P.run_kat(case, P.PncModel(case["replicas"], max_emit=2))
    assert len(got) == len(want)
    for i, (g, m) in enumerate(zip(got, want)):
        assert np.array_equal(g, m), f"{case['name']}: after op {i}: engine {[P.from_words(x) for x in g]} model {[P.from_words(x) for x in m]}"


# ------------------------------------------------------------------ 2. crafted two-replica merges
U32, U64 = 1 << 32, 1 << 64


def one_key(node, key, version, slots, vv=None):
    """A replica of `node` that counted `key` once (birth dot node -> version), with the given 16 slots."""
    return P.PNCounterMap(M.ORSet({key: {node: version}}, vv or {node: version}), {key: tuple(slots)})


def pairs(lo_side, hi_side):
    """16 slots for either side from 8 (smaller, larger) pairs: the larger value alternates between the sides."""
    a = [hi_side[i // 2] if i % 2 == 0 else lo_side[i // 2] for i in range(16)]
    b = [lo_side[i // 2] if i % 2 == 0 else hi_side[i // 2] for i in range(16)]
    return a, b


def rand_slots(rng):
    return tuple(int(x) | 1 for x in rng.integers(0, U64, 16, dtype=np.uint64))


def dots_map(total, phase, rng):
    """`total` live dots in all (1, 2, 3 or 5: the row's dots section is rounded up to 4 u32), on nodes of
    `phase`'s parity, so that two phases are concurrent and keep all their dots."""
    shape = {1: [(10, 1)], 2: [(10, 1), (50, 1)], 3: [(10, 2), (50, 1)], 5: [(10, 2), (20, 2), (63, 1)]}[total]
    dots = {key: {phase + 2 * i: 1 + phase + i for i in range(c)} for key, c in shape}
    vv = {}
    for d in dots.values():
        for n, v in d.items():
            vv[n] = max(vv.get(n, 0), v)
    return P.PNCounterMap(M.ORSet(dots, vv), {key: rand_slots(rng) for key in dots})


def full_map(phase, rng):
    """All 64 keys live with 8 dots each and 16 non-zero slots; the version vector equals the dots, so two
    phases are Concurrent and every dot of both sides survives as the larger one."""
    dots = {n: (5 if (n + phase) % 2 == 0 else 3) for n in range(P.NODES)}
    return P.PNCounterMap(M.ORSet({k: dict(dots) for k in range(P.ELEMS)}, dots), {k: rand_slots(rng) for k in range(P.ELEMS)})


def row_u32(m):
    """The used length of m's snapshot row: header, the live dots rounded up to 4, 32 u32 per live key."""
    dots = sum(len(d) for d in m.keys.elements.values())
    return 32 + (dots + 3) // 4 * 4 + 32 * len(m.values)


def merge_cases():
    out = []
    sm = [(i + 1) << 32 | 0x80000000 + i for i in range(8)]
    a, b = pairs(sm, [x + (3 << 32) for x in sm])
    out.append(("high_u32_differs", one_key(0, 3, 1, a), one_key(1, 3, 1, b)))
    a, b = pairs(sm, [x + 5 for x in sm])
    out.append(("low_u32_differs", one_key(0, 3, 1, a), one_key(1, 3, 1, b)))
    # across 2^32: the smaller value has the larger low word
    a, b = pairs([U32 - 1 - i for i in range(8)], [U32 + i for i in range(8)])
    out.append(("across_2_32", one_key(0, 60, 1, a), one_key(1, 60, 1, b)))
    a, b = pairs([U64 - 2, 0, U32 - 1, U64 - U32, 1, U64 - 2, U64 >> 1, (U64 >> 1) - 1], [U64 - 1] * 8)
    out.append(("at_2_64_minus_1", one_key(0, 31, 1, a), one_key(1, 31, 1, b)))
    rng = np.random.default_rng(12)
    # a key live on one side only, not dominated: taken over with all 16 slots
    out.append(("one_side_not_dominated", one_key(0, 5, 4, rand_slots(rng)), one_key(1, 44, 2, rand_slots(rng))))
    # a key live on one side only and dominated by the other's version vector: dropped, 16 zeros left
    seen = P.PNCounterMap(M.ORSet({44: {1: 2}}, {0: 4, 1: 2}), {44: rand_slots(rng)})
    out.append(("one_side_dominated", one_key(0, 5, 4, rand_slots(rng)), seen))
    out.append(("key_0_vs_key_63", one_key(0, 0, 1, rand_slots(rng)), one_key(1, 63, 1, rand_slots(rng))))
    for total in (1, 2, 3, 5):
        out.append((f"live_dots_{total}", dots_map(total, 0, rng), dots_map(total, 1, rng)))
    out.append(("all_64_keys_8_dots", full_map(0, rng), full_map(1, rng)))
    return out


MERGES = merge_cases()


@pytest.mark.parametrize("case", MERGES, ids=[c[0] for c in MERGES])
def test_crafted_merges_both_directions(built, pipeline, case):
    name, a, b = case
    init = np.stack([P.to_words(a), P.to_words(b)])
    if name == "all_64_keys_8_dots":  # the row fills the whole pitch
        assert all(len(m.values) == 64 and all(len(d) == 8 for d in m.keys.elements.values()) and
                   all(all(s) for s in m.values.values()) and row_u32(m) == 2592 for m in (a, b))
    if name.startswith("live_dots_"):
        assert all(sum(len(d) for d in m.keys.elements.values()) == int(name[10:]) for m in (a, b))
    maps = [a, b]
    for sender in (0, 1):
        w = workload(name, 2, init, [sender], [Op.make(Op.GOSSIP, 0)])
        sg, words, model = run_both(w, f"{name} sender {sender}")
        want = maps[1 - sender].merge(maps[sender])
        assert P.from_words(words[1 - sender]) == want and P.from_words(words[sender]) == maps[sender], name
        assert sg.unhandled == 0 and sg.in_flight == 0
        if name in ("high_u32_differs", "low_u32_differs", "across_2_32", "at_2_64_minus_1"):
            key = next(iter(a.values))
            assert want.values[key] == tuple(max(x, y) for x, y in zip(a.values[key], b.values[key]))
            assert want.values[key] != a.values[key] and want.values[key] != b.values[key]
    if name == "one_side_not_dominated":
        assert a.merge(b).values == {5: a.values[5], 44: b.values[44]}
    if name == "one_side_dominated":
        assert a.merge(b).values == {44: b.values[44]} and b.merge(a).values == {44: b.values[44]}  # key 5 dropped
    if name == "key_0_vs_key_63":
        assert set(a.merge(b).values) == {0, 63}


# ------------------------------------------------------------------ 3. ops on 16 replicas
def test_increment_by_zero_creates_the_key_and_nodes_wrap(built, pipeline):
    """PNCounter.change by 0 leaves the counter, ORMap.updated still adds the key; replicas 8..15 count into the
    slots of node id % 8 (replica 9 and replica 1 both write node 1's slots and dots)."""
    dst = [3, 3, 9, 1, 12, 15, 15]
    pay = [Op.increment_key(7, 0), Op.decrement_key(8, 0), Op.increment_key(2, 11), Op.increment_key(2, 5),
           Op.decrement_key(63, 4), Op.increment_key(0, (1 << 18) - 1), Op.decrement_key(0, 1)]
    w = workload("zero_and_wrap", 16, None, dst, pay, throughput=8)
    sg, words, model = run_both(w, "zero and wrap")
    m = [P.from_words(x) for x in words]
    assert m[3].entries == {7: 0, 8: 0} and m[3].keys.elements == {7: {3: 1}, 8: {3: 2}} and m[3].values[7] == P.ZERO
    assert m[9].values[2][1] == 11 and m[9].keys.elements[2] == {1: 1} and m[1].values[2][1] == 5
    assert m[12].values[63][8 + 4] == 4 and m[12].entries == {63: -4}
    assert m[15].values[0][7] == (1 << 18) - 1 and m[15].values[0][8 + 7] == 1 and sg.unhandled == 0


def test_snapshot_sees_the_state_at_its_position(built, pipeline):
    """inc, remove, inc, gossip, inc in one run of one replica (throughput 8): the snapshot row carries the state
    after the third message, the replica ends with the fifth applied."""
    seed = 1
    peer = crdt_peer(seed, 5, 0, 0, 16)
    pay = [Op.increment_key(4, 10), Op.make(Op.REMOVE, 4), Op.increment_key(4, 3), Op.make(Op.GOSSIP, 0), Op.increment_key(4, 2)]
    w = workload("snapshot_position", 16, None, [5] * 5, pay, throughput=8, seed=seed)
    sg, words, model = run_both(w, "snapshot position")
    own, got = P.from_words(words[5]), P.from_words(words[peer])
    assert got.entries == {4: 3} and got.keys.elements == {4: {5: 2}} and got.keys.vvector == {5: 2}
    assert own.entries == {4: 5} and own.keys.elements == {4: {5: 3}} and sg.delivered == 6


# a gossip seed for which replica 2's tick goes to PEER and PEER's tick comes back to replica 2
ANOMALY_SEED = next(s for s in range(1, 4000) if crdt_peer(s, crdt_peer(s, 2, 0, 0, 16), 0, 0, 16) == 2)


def test_recount_after_remove_gets_old_slots_back_from_a_stale_peer(built, pipeline):
    """ORMap.dryMerge merges the values before it knows which dots survive: replica 2 counts key 9 to 5 - 2 and
    gossips; removes the key and counts it again by 1; the peer, which still holds the old counter, gossips back.
    Key 9 then lives on the new dot with the old slots: 3, not 1 (tests/test_pncountermap_model.py pins the same
    on the model).  Reproduced, not repaired."""
    peer = crdt_peer(ANOMALY_SEED, 2, 0, 0, 16)
    w = workload("anomaly", 16, None, [2, 2, 2], [Op.increment_key(9, 5), Op.decrement_key(9, 2), Op.make(Op.GOSSIP, 0)],
                 throughput=8, seed=ANOMALY_SEED)

    def drive(t):
        t.run()
        t.tell([2, 2], [Op.make(Op.REMOVE, 9), Op.increment_key(9, 1)])
        t.run()
        t.tell([peer], [Op.make(Op.GOSSIP, 0)])
        return t.run()

    sg, words, model = run_both(w, "anomaly", drive)
    got = P.from_words(words[2])
    assert got.keys.elements == {9: {2: 3}} and got.entries == {9: 3} and got.values[9][2] == 5 and got.values[9][8 + 2] == 2
    assert P.from_words(words[peer]).entries == {9: 3} and P.from_words(words[peer]).keys.elements == {9: {2: 2}}


@pytest.mark.parametrize("what", ["slot", "version"])
def test_range_errors(built, pipeline, what):
    """A slot that would pass 2^64 - 1 (the reference's BigInt would not wrap) and a version that would pass
    2^32 - 1 (the reference's Long would not) raise AGX_ERANGE."""
    if what == "slot":
        init0 = one_key(3, 6, 1, [0, 0, 0, U64 - 1] + [0] * 12)
        with pytest.raises(P.SlotRange):
            init0.change(3, 6, 1)
    else:
        init0 = one_key(3, 6, U32 - 1, [1] * 16)
    init = np.zeros((16, W), np.uint64)
    init[3] = P.to_words(init0)
    eng = GpuEngine(EngineConfig(n_actors=16, n_words=W, max_emit=2, bucket_actors=32, msg_capacity=CAP))
    try:
        eng.register_range(0, 16, Kind.PNCOUNTERMAP, init)
        eng.set_gossip(1, 1)
        eng.tell([3], [Op.increment_key(6, 0)] if what == "slot" else [Op.increment_key(7, 1)])
        if what == "slot":  # (by 0 at 2^64 - 1: no change, no error; the version moves on)
            eng.run()
            assert P.from_words(eng.read_state()[0][3]).values[6][3] == U64 - 1
            eng.tell([3], [Op.increment_key(6, 1)])
        with pytest.raises(AgxError) as ei:
            eng.run()
        assert ei.value.status == AGX_ERANGE
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. seeded runs against the BSP model
def writers_merge(w):
    """merge_all of the eight writers' maps after their round-0 ops alone."""
    m = P.PncModel(n_actors=w.n_actors)
    m.register_range(0, w.n_actors, Kind.PNCOUNTERMAP)
    d, _, p = w.tells
    m.tell(d[:160], p[:160])
    m.run()
    return P.merge_all(m.maps[:8])


def census(model):
    """What a seeded case is for: rows stayed queued past a tick, a key was removed and created again, a
    both-sides merge changed a slot."""
    assert model.queued_gossips > 0, model.queued_gossips
    assert model.recreated > 0, model.recreated
    assert model.merge_census.get("both_sides_changed", 0) > 0, model.merge_census


def converged_on(w):
    expected = writers_merge(w)

    def check(model):
        census(model)
        assert model.converged() and all(m == expected for m in model.maps) and len(expected.values) > 3
        assert model.c["in_flight"] == 0 and model.c["unhandled"] == 0
    return check


SEEDED = {
    "throughput_5": (dict(n=48, rounds=12, throughput=5), None),
    "throughput_1_poison_0": (dict(n=40, rounds=16, throughput=1), "0"),
    "throughput_1_poison_255": (dict(n=40, rounds=16, throughput=1), "255"),
    "bounded_mailbox": (dict(n=40, rounds=16, throughput=1, capacity=21), None),
}


@pytest.mark.parametrize("case", list(SEEDED))
def test_seeded_runs_converge_to_the_writers_merge(built, pipeline, monkeypatch, case):
    """Eight writers collide on a dozen keys, removes among their counts; every replica gossips to 2 peers a tick.
    At throughput 1 gossips wait in the mailboxes for many ticks and their rows are copied forward each superstep
    by their used length -- with the heap poisoned, a row word read and never written shows; a mailbox of 21 holds
    a writer's 20 ops and its tick and tail-drops gossips behind them."""
    kw, poison = SEEDED[case]
    if poison is not None:
        monkeypatch.setenv("AGX_HEAP_POISON", poison)
    w = wl.crdt_pncountermap(fanout=2, bucket_actors=32, **kw)
    check = converged_on(w)

    def check_case(model):
        check(model)
        if kw["throughput"] == 1:
            assert model.queued_gossips > 1000, model.queued_gossips
        if kw.get("capacity"):
            assert model.tail_dropped_gossips > 0 and model.c["dead_letters"] > 0
    sg, words, _ = run_both(w, case, check=check_case)
    assert all(np.array_equal(words[a, :W], words[0, :W]) for a in range(kw["n"]))


def test_three_runs_with_host_writes_between(built, pipeline):
    """Runs that stop on their superstep budget, host counts and removes staged in between -- one of them removes
    a key and counts it again while peers still hold its old counter."""
    w = wl.crdt_pncountermap(40, rounds=14, fanout=2, bucket_actors=32)

    def drive(t):
        t.run(3)
        t.tell([0, 9, 9, 17, 39], [Op.increment_key(2, 500), Op.decrement_key(2, 501), Op.make(Op.REMOVE, 3),
                                   Op.increment_key(50, 502), Op.increment_key(2, 0)])
        t.run(4)
        t.tell([8, 0, 0, 33], [Op.increment_key(2, 600), Op.make(Op.REMOVE, 2), Op.increment_key(2, 1), Op.decrement_key(63, 601)])
        t.run(0)  # (a run without mail to drain)
        return t.run()

    def check(model):
        census(model)
        assert model.converged() and model.c["in_flight"] == 0 and model.c["supersteps"] > 7 and len(model.maps[20].values) > 3

    run_both(w, "three runs", drive, check)


def test_hot_bucket_takes_the_skew_launch(built, pipeline):
    """2112 host counts for the 32 replicas of bucket 0 beside the writers' ops and the ticks: that bucket's first
    inbox is more than one tile of 2048 messages, which is what sends a bucket to the skew launch (by
    construction: the model's per-bucket inbox census).  At throughput 20 those replicas drain their 66 counts
    over four supersteps, their ticks behind them and the gossips of the others behind those, so rows queue
    there as well."""
    w = wl.crdt_pncountermap(64, rounds=12, fanout=2, throughput=20, bucket_actors=32)
    d, s, p = w.tells
    hot = np.repeat(np.arange(32, dtype=np.uint32), 66)
    j = np.arange(hot.size, dtype=np.uint32)
    ops = np.array([(Op.increment_key if x % 3 else Op.decrement_key)(int(x * 7 % 12), int(x % 1000)) for x in j], np.uint32)
    k = 160  # (after the writers' ops, before the ticks)
    w.tells = (np.concatenate([d[:k], hot, d[k:]]), np.concatenate([s[:k], np.full(hot.size, NO_SENDER, np.uint32), s[k:]]),
               np.concatenate([p[:k], ops, p[k:]]))

    def check(model):
        assert model.max_bucket_inbox(32) > 2048, model.max_bucket_inbox(32)
        census(model)
        assert model.converged() and model.c["in_flight"] == 0 and model.c["unhandled"] == 0

    run_both(w, "hot bucket", check=check, msg_capacity=4096)
