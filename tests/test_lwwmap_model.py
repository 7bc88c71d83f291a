"""The LWWMap model (tests/lwwmap_model.py) against the reference's known answers
(tests/golden/lwwmap_kats.json), the join laws on reachable states, the canonical form, the words
round trip of akka_amd.ddata.LWWMap and the workload builder.  No GPU."""
import json
import pathlib
import random

import numpy as np
import pytest

from akka_amd import ddata
from akka_amd import workloads as wl
from akka_amd.engine import CRDT_WORDS, Kind, Op
from tests import lwwmap_model as L

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "lwwmap_kats.json").read_text())["cases"]


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_model_against_the_kats(case):
    assert pathlib.PurePosixPath(case["spec"]).name in ("LWWMapSpec.scala", "LWWRegisterSpec.scala", "ORMapSpec.scala")
    assert case["line"] > 0
    m = L.LwwModel(case["replicas"], max_emit=2)
    trace = L.run_kat(case, m)
    assert trace and all(L.from_words(w).canonical() for t in trace for w in t)


def test_kats_cover_the_listed_specs():
    by = {(pathlib.PurePosixPath(c["spec"]).name, c["line"]) for c in KATS}
    assert {("LWWMapSpec.scala", 22), ("LWWMapSpec.scala", 27), ("LWWMapSpec.scala", 37), ("LWWMapSpec.scala", 46),
            ("LWWRegisterSpec.scala", 21), ("LWWRegisterSpec.scala", 30), ("LWWRegisterSpec.scala", 47),
            ("LWWRegisterSpec.scala", 59), ("ORMapSpec.scala", 72), ("ORMapSpec.scala", 97),
            ("ORMapSpec.scala", 136)} <= by


SHARED_KEYS = (20, 31, 32)


def owned_keys(node: int):
    return (node, 56 + node)


def reachable_pool(seed: int, clock=L.default_clock, n_ops: int = 200, removes: bool = True):
    """States of one history: 8 writers (one per node) put and remove and merge one another, sibling
    replicas copy, remove and merge; logical time advances with every op, so that a node never writes
    one key twice at one timestamp.

    Removes follow one discipline: a key that is ever removed is written by one node only (`owned_keys`),
    and the keys every node writes (SHARED_KEYS) are never removed.  Without it the reference's ORMap is
    not associative: a remove concurrent with another node's put of the same key can leave the key alive
    with the register of the removed lineage, depending on the merge order
    (test_ormap_remove_concurrent_with_a_put_is_order_dependent pins the example).  Under the reverse
    clock the earlier write wins, so the register of a removed lineage beats its own node's later put as
    well: that pool has no removes (`removes=False`: a put takes the place of each)."""
    rng = random.Random(seed)
    W = [L.LWWMap() for _ in range(L.NODES)]
    pool = [L.LWWMap()]
    for now in range(1, n_ops + 1):
        k = rng.randrange(L.NODES)
        r = rng.random()
        if r < 0.45:
            W[k] = W[k].put(k, rng.choice(owned_keys(k) + SHARED_KEYS), rng.randrange(1 << 18), clock, now)
        elif r < 0.60 and removes:
            W[k] = W[k].remove(rng.choice(owned_keys(k)))
        elif r < 0.60:
            W[k] = W[k].put(k, rng.choice(owned_keys(k)), rng.randrange(1 << 18), clock, now)
        elif r < 0.85:
            W[k] = W[k].merge(W[rng.randrange(L.NODES)])
        else:
            s = W[k].copy()
            if removes:
                s = s.remove(rng.choice(owned_keys(rng.randrange(L.NODES))))
            pool.append(s.merge(W[rng.randrange(L.NODES)]))
        assert W[k].canonical()
        if now % 5 == 0:
            pool.append(W[k].copy())
    return pool + [w.copy() for w in W]


def test_ormap_remove_concurrent_with_a_put_is_order_dependent():
    """The reference's ORMap.dryMerge (DD/ORMap.scala:379-404) merges the values of a key present on both
    sides before it knows which dots survive: b's register can outlive b's dots.  a = node 1 put key 2;
    b = node 2 put key 2 later; c saw b's put and removed the key.  (a merge b) merge c keeps the key on
    a's dot with b's newer register; a merge (b merge c) keeps a's register.  Both are what the Scala
    code computes; the model restates it, the engine follows the model."""
    a = L.LWWMap().put(1, 2, 111, L.default_clock, 37)
    b = L.LWWMap().put(2, 2, 222, L.default_clock, 50)
    c = b.remove(2)
    left, right = a.merge(b).merge(c), a.merge(b.merge(c))
    assert left.keys == right.keys and left.keys.elements == {2: {1: 1}}
    assert left.values[2] == (2, 222, 50) and right.values[2] == (1, 111, 37)
    assert left.merge(right) == right.merge(left) and left.merge(right).values[2] == (2, 222, 50)  # gossip still converges


@pytest.mark.parametrize("clock", ["default", "reverse"])
def test_merge_is_a_join_on_reachable_states(clock):
    pool = reachable_pool(0x5EED, L.CLOCKS[clock], removes=clock == "default")
    assert len(pool) > 40 and max(len(m.values) for m in pool) >= 8
    rng = random.Random(7)
    for m in pool:
        assert m.merge(m) == m and m.canonical()
    for _ in range(600):
        a, b, c = rng.choice(pool), rng.choice(pool), rng.choice(pool)
        ab = a.merge(b)
        assert ab == b.merge(a)
        assert ab.merge(c) == a.merge(b.merge(c))
        assert ab.canonical()
        assert np.array_equal(L.to_words(L.from_words(L.to_words(ab))), L.to_words(ab))


def test_canonical_form_after_every_op():
    m = L.LWWMap().put(0, 5, 9, L.default_clock, 1)
    assert L.to_words(m)[L.TS_WORD + 5] == 1 and L.to_words(m).view(np.uint32)[L.REG_U32 + 5] == 9
    r = m.remove(5)
    assert r.canonical() and not L.to_words(r)[L.TS_WORD:].any()      # register cleared with the key
    assert L.to_words(r)[:L.TS_WORD].any()                             # ... the version vector stays
    again = r.put(0, 5, 3, L.default_clock, 7)
    assert again.values[5] == (0, 3, 7)                                # a put after a remove restarts at clock(0)
    # a merge that drops a key: `seen` saw the put and removed the key, so its vvector dominates the dot
    seen = m.remove(5)
    assert m.merge(seen).canonical() and m.merge(seen).entries == {} and not L.to_words(m.merge(seen))[L.TS_WORD:].any()
    with pytest.raises(L.TimestampRange):
        L.LWWMap(m.keys, {5: (0, 9, L.INT64_MAX)}).put(0, 5, 1, L.default_clock, 1)
    with pytest.raises(L.TimestampRange):
        L.LWWMap(m.keys, {5: (0, 9, L.INT64_MIN)}).put(0, 5, 1, L.reverse_clock, 1)


def test_reverse_clock_is_first_write_wins():
    a = L.LWWMap().put(0, 1, 10, L.reverse_clock, 100)
    b = L.LWWMap().put(1, 1, 20, L.reverse_clock, 200)
    assert a.values[1][2] == -100 and b.values[1][2] == -200
    assert a.merge(b).entries == {1: 10} and b.merge(a).entries == {1: 10}


def test_ddata_words_round_trip():
    pool = reachable_pool(11)
    for m in pool:
        w = L.to_words(m)
        d = ddata.LWWMap.from_words(w)
        assert d.entries == m.entries and d.size == len(m.values)
        for k, (node, value, ts) in m.values.items():
            assert d.contains(k) and d.get(k) == value and d.timestamp(k) == ts and d.updated_by(k) == node
        assert not d.contains(62) or 62 in m.values
        assert d.get(40) is None and d.timestamp(40) is None and d.updated_by(40) is None
        assert np.array_equal(d.to_words(), w)
    neg = L.LWWMap().put(3, 63, (1 << 18) - 1, L.reverse_clock, 1 << 40)
    d = ddata.LWWMap.from_words(L.to_words(neg))
    assert d.timestamp(63) == -(1 << 40) and d.get(63) == (1 << 18) - 1 and d.updated_by(63) == 3
    bad = L.to_words(neg)
    bad[L.TS_WORD + 1] = 5  # a register without a live dot
    with pytest.raises(ValueError):
        ddata.LWWMap.from_words(bad)
    with pytest.raises(ValueError):
        ddata.LWWMap.from_words(np.zeros(260, np.uint64))


def test_op_put_encoding():
    assert Op.put(63, (1 << 18) - 1) == (Op.PUT << 24) | 0xFFFFFF
    assert Op.put(5, 9) == (8 << 24) | 5 | (9 << 6)
    for key, value in ((64, 0), (-1, 0), (0, 1 << 18), (0, -1)):
        with pytest.raises(ValueError):
            Op.put(key, value)
    assert CRDT_WORDS[Kind.LWWMAP] == 356 and Kind.LWWMAP == 11


def test_workload_builder():
    w = wl.crdt_lwwmap(96, rounds=4, fanout=2, puts_per_writer=16, removes=4, bucket_actors=32, clock="reverse", base=77)
    assert w.n_actors == 96 and w.n_words == 356 and w.max_emit == 3 and w.bucket_actors == 32
    assert w.ranges == [(0, 96, Kind.LWWMAP, None)] and w.gossip == (2, wl.SEED) and w.lwwmap == ("reverse", 77)
    dst, src, pay = w.tells
    ops = pay[:8 * 20]
    assert (dst[:160] == np.repeat(np.arange(8), 20)).all() and (dst[160:] == np.arange(96)).all()
    assert ((ops >> 24) == Op.PUT).sum() == 8 * 16 and ((ops >> 24) == Op.REMOVE).sum() == 8 * 4
    assert (pay[160:] == Op.make(Op.GOSSIP, 3)).all()
    keys = np.where((ops >> 24) == Op.PUT, ops & 63, ops & 0xFFFFFF)
    assert keys.max() < 12                                         # few keys ...
    put_keys = [set((ops[20 * a:20 * a + 20][(ops[20 * a:20 * a + 20] >> 24) == Op.PUT] & 63).tolist()) for a in range(8)]
    assert any(put_keys[a] & put_keys[b] for a in range(8) for b in range(a))  # ... so writers collide on keys
    assert wl.crdt_lwwmap(4).n_actors == 4 and len(wl.crdt_lwwmap(4).tells[0]) == 4 * 20 + 4
    # the model runs it to quiescence and converges on the writers' merge
    m = L.LwwModel(**wl.crdt_lwwmap(24, rounds=12, bucket_actors=32).engine_kwargs())
    wl.crdt_lwwmap(24, rounds=12, bucket_actors=32).apply_to(m)
    st = m.run()
    assert st["in_flight"] == 0 and st["unhandled"] == 0 and m.converged() and len(m.maps[0].values) > 3
