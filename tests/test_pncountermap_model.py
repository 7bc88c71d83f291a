"""The PNCounterMap model (tests/pncountermap_model.py) against the reference's known answers
(tests/golden/pncountermap_kats.json), the join laws on reachable states, the resurrect-after-remove
order dependence, the canonical form, the words round trip of akka_amd.ddata.PNCounterMap, the Op
range checks and the workload builder.  No GPU."""
import json
import pathlib
import random

import numpy as np
import pytest

from akka_amd import ddata
from akka_amd import workloads as wl
from akka_amd.engine import CRDT_DELTA_WORDS, CRDT_WORDS, Kind, Op
from tests import pncountermap_model as P

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "pncountermap_kats.json").read_text())["cases"]


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_model_against_the_kats(case):
    assert pathlib.PurePosixPath(case["spec"]).name == "PNCounterMapSpec.scala" and case["line"] > 0
    trace = P.run_kat(case, P.PncModel(case["replicas"], max_emit=2))
    assert trace and all(P.from_words(w).canonical() for t in trace for w in t)


def test_kats_cover_the_listed_specs():
    by = [(pathlib.PurePosixPath(c["spec"]).name, c["line"]) for c in KATS]
    assert {("PNCounterMapSpec.scala", 27), ("PNCounterMapSpec.scala", 32), ("PNCounterMapSpec.scala", 42),
            ("PNCounterMapSpec.scala", 51)} <= set(by)
    assert by.count(("PNCounterMapSpec.scala", 32)) == 2  # merged both ways


SHARED_KEYS = (20, 31, 32)


def owned_keys(node: int):
    return (node, 56 + node)


def reachable_pool(seed: int, n_ops: int = 240):
    """States of one history: 8 writers (one per node) count, remove and merge one another, sibling replicas
    copy and merge.

    Removes follow one discipline: a key that is ever removed is counted by one node only (`owned_keys`), the
    keys every node counts (SHARED_KEYS) are never removed -- no remove is concurrent with another node's count
    of the same key --, and a removed key is not counted again.  Without the first the reference's ORMap is not
    associative (test_remove_concurrent_with_a_count_is_order_dependent); without the second a stale copy
    gives the key's old slots back (test_recount_after_remove_gets_old_slots_back), which is order dependent
    as well: (old merge removed) merge recounted has the new slots, old merge (removed merge recounted) the
    old ones."""
    rng = random.Random(seed)
    W = [P.PNCounterMap() for _ in range(P.NODES)]
    dead = [set() for _ in range(P.NODES)]
    pool = [P.PNCounterMap()]
    for i in range(1, n_ops + 1):
        k = rng.randrange(P.NODES)
        r = rng.random()
        if r < 0.50:
            keys = [x for x in owned_keys(k) if x not in dead[k]] + list(SHARED_KEYS)
            n = rng.choice((0, 1, rng.randrange(1 << 18)))
            W[k] = W[k].change(k, rng.choice(keys), n if rng.random() < 0.7 else -n)
        elif r < 0.58:
            key = rng.choice(owned_keys(k))
            dead[k].add(key)
            W[k] = W[k].remove(key)
        elif r < 0.85:
            W[k] = W[k].merge(W[rng.randrange(P.NODES)])
        else:
            pool.append(W[k].copy().merge(W[rng.randrange(P.NODES)]))
        assert W[k].canonical()
        if i % 5 == 0:
            pool.append(W[k].copy())
    return pool + [w.copy() for w in W]


def test_remove_concurrent_with_a_count_is_order_dependent():
    """The reference's ORMap.dryMerge (DD/ORMap.scala:379-404) merges the values of a key present on both
    sides before it knows which dots survive.  a = node 1 counted key 2 by 7; b = node 2 counted it by 9;
    c saw b's count and removed the key.  (a merge b) merge c keeps the key on a's dot with both nodes' slots;
    a merge (b merge c) keeps a's slots alone.  Both are what the Scala code computes."""
    a = P.PNCounterMap().change(1, 2, 7)
    b = P.PNCounterMap().change(2, 2, 9)
    c = b.remove(2)
    left, right = a.merge(b).merge(c), a.merge(b.merge(c))
    assert left.keys == right.keys and left.keys.elements == {2: {1: 1}}
    assert left.entries == {2: 16} and right.entries == {2: 7}
    assert left.merge(right) == right.merge(left) and left.merge(right).entries == {2: 16}  # gossip still converges


def test_recount_after_remove_gets_old_slots_back():
    """A key removed and counted again on one replica: the fresh counter starts at 0 (ORMap.updated on an absent
    key), but a peer that still holds the old counter gives the old slots back, since the key is on both sides
    and PNCounter.merge takes the slot-wise maximum.  Pinned, not repaired."""
    a = P.PNCounterMap().change(0, 2, 5).change(0, 2, -2)
    stale = a.copy()
    again = a.remove(2).change(0, 2, 1)
    assert again.entries == {2: 1} and again.values[2] == (1,) + (0,) * 15 and again.keys.elements[2] == {0: 3}
    merged = again.merge(stale)
    assert merged.keys.elements == {2: {0: 3}} and merged.entries == {2: 3}      # max(1, 5) - max(0, 2), not 1
    assert stale.merge(again) == merged
    removed = a.remove(2)
    assert stale.merge(removed).merge(again).entries == {2: 1}                   # ... and the order decides
    assert stale.merge(removed.merge(again)).entries == {2: 3}


def test_merge_is_a_join_on_reachable_states():
    pool = reachable_pool(0x5EED)
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
        assert np.array_equal(P.to_words(P.from_words(P.to_words(ab))), P.to_words(ab))


def test_canonical_form_after_every_op():
    m = P.PNCounterMap().change(3, 5, 9).change(3, 5, -4)
    w = P.to_words(m)
    assert w[P.CTR_WORD + 16 * 5 + 3] == 9 and w[P.CTR_WORD + 16 * 5 + 8 + 3] == 4 and not w[260:272].any()
    assert int(w[P.CTR_WORD:].sum()) == 13
    zero = P.PNCounterMap().change(0, 7, 0)                         # an increment by 0 creates the key with value 0
    assert zero.canonical() and zero.entries == {7: 0} and zero.keys.elements == {7: {0: 1}}
    r = m.remove(5)
    assert r.canonical() and not P.to_words(r)[P.CTR_WORD:].any()   # slots cleared with the key
    assert P.to_words(r)[:260].any()                                # ... the version vector stays
    assert r.change(3, 5, 2).values[5] == (0, 0, 0, 2) + (0,) * 12  # a count after a remove starts a fresh counter
    seen = m.remove(5)  # saw the count and removed the key: its vvector dominates the dot
    assert m.merge(seen).canonical() and m.merge(seen).entries == {} and not P.to_words(m.merge(seen))[P.CTR_WORD:].any()
    full = P.PNCounterMap(m.keys, {5: (P.U64_MAX,) * 16})
    assert full.change(3, 5, 0) .values[5] == (P.U64_MAX,) * 16     # by 0: no change, no range error
    with pytest.raises(P.SlotRange):
        full.change(3, 5, 1)
    with pytest.raises(P.SlotRange):
        full.change(3, 5, -1)


def test_ddata_words_round_trip():
    for m in reachable_pool(11):
        w = P.to_words(m)
        d = ddata.PNCounterMap.from_words(w)
        assert d.entries == m.entries and d.size == len(m.values)
        for k, slots in m.values.items():
            assert d.contains(k) and d.get(k) == P.counter_value(slots)
            assert d.increments(k) == {n: slots[n] for n in range(8) if slots[n]}
            assert d.decrements(k) == {n: slots[8 + n] for n in range(8) if slots[8 + n]}
        assert d.get(40) is None and d.increments(40) is None and d.decrements(40) is None and not d.contains(40)
        assert np.array_equal(d.to_words(), w)
    neg = P.PNCounterMap().change(3, 63, -5).change(3, 63, 2)
    d = ddata.PNCounterMap.from_words(P.to_words(neg))
    assert d.get(63) == -3 and d.entries == {63: -3} and isinstance(d.get(63), int)
    big = P.PNCounterMap(neg.keys, {63: (P.U64_MAX,) * 8 + (0,) * 8})
    assert ddata.PNCounterMap.from_words(P.to_words(big)).get(63) == 8 * P.U64_MAX  # (a Python int: no wrap)
    bad = P.to_words(neg)
    bad[P.CTR_WORD + 16] = 5  # slots without a live dot
    with pytest.raises(ValueError):
        ddata.PNCounterMap.from_words(bad)
    bad = P.to_words(neg)
    bad[265] = 1  # the padding
    with pytest.raises(ValueError):
        ddata.PNCounterMap.from_words(bad)
    with pytest.raises(ValueError):
        ddata.PNCounterMap.from_words(np.zeros(356, np.uint64))


def test_op_count_encoding():
    assert Op.increment_key(63, (1 << 18) - 1) == (Op.INCREMENT << 24) | 0xFFFFFF
    assert Op.decrement_key(5, 9) == (2 << 24) | 5 | (9 << 6)
    assert Op.increment_key(0, 0) == 1 << 24
    for f in (Op.increment_key, Op.decrement_key):
        for key, n in ((64, 0), (-1, 0), (0, 1 << 18), (0, -1)):
            with pytest.raises(ValueError):
                f(key, n)
    assert CRDT_WORDS[Kind.PNCOUNTERMAP] == 1296 and Kind.PNCOUNTERMAP == 12
    assert Kind.PNCOUNTERMAP not in CRDT_DELTA_WORDS and Kind.LWWMAP not in CRDT_DELTA_WORDS


def test_workload_builder():
    w = wl.crdt_pncountermap(96, rounds=4, fanout=2, incs_per_writer=16, removes=4, bucket_actors=32)
    assert w.n_actors == 96 and w.n_words == 1296 and w.max_emit == 3 and w.bucket_actors == 32
    assert w.ranges == [(0, 96, Kind.PNCOUNTERMAP, None)] and w.gossip == (2, wl.SEED) and w.lwwmap is None
    dst, src, pay = w.tells
    ops = pay[:8 * 20]
    assert (dst[:160] == np.repeat(np.arange(8), 20)).all() and (dst[160:] == np.arange(96)).all()
    code = ops >> 24
    assert ((code == Op.INCREMENT) | (code == Op.DECREMENT)).sum() == 8 * 16 and (code == Op.REMOVE).sum() == 8 * 4
    assert (code == Op.INCREMENT).sum() > (code == Op.DECREMENT).sum() > 0
    assert (pay[160:] == Op.make(Op.GOSSIP, 3)).all()
    keys = np.where(code == Op.REMOVE, ops & 0xFFFFFF, ops & 63)
    assert keys.max() < 12                                         # few keys ...
    cnt_keys = [set((ops[20 * a:20 * a + 20][code[20 * a:20 * a + 20] != Op.REMOVE] & 63).tolist()) for a in range(8)]
    assert any(cnt_keys[a] & cnt_keys[b] for a in range(8) for b in range(a))  # ... so writers collide on keys
    assert wl.crdt_pncountermap(4).n_actors == 4 and len(wl.crdt_pncountermap(4).tells[0]) == 4 * 20 + 4
    assert np.array_equal(wl.pncountermap_ops(8, 16, 4), ops.reshape(8, 20))
    # the model runs it to quiescence and converges
    m = P.PncModel(**wl.crdt_pncountermap(24, rounds=12, bucket_actors=32).engine_kwargs())
    wl.crdt_pncountermap(24, rounds=12, bucket_actors=32).apply_to(m)
    st = m.run()
    assert st["in_flight"] == 0 and st["unhandled"] == 0 and m.converged() and len(m.maps[0].values) > 3
