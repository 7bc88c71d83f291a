"""The ORMultiMap model (tests/ormultimap_model.py) against the reference's known answers
(tests/golden/ormultimap_kats.json), every op rule, the two anomalies the reference documents, the join laws on
histories without key removal, the canonical form, the words round trip of akka_amd.ddata.ORMultiMap, the Op range
checks and the workload builder.  No GPU."""
import json
import pathlib
import random

import numpy as np
import pytest

from akka_amd import ddata
from akka_amd import workloads as wl
from akka_amd.engine import CRDT_DELTA_WORDS, CRDT_WORDS, Kind, Op
from tests import crdt_model as M
from tests import ormultimap_model as P

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "ormultimap_kats.json").read_text())["cases"]
E = P.ORMultiMap


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_model_against_the_kats(case):
    assert pathlib.PurePosixPath(case["spec"]).name == "ORMultiMapSpec.scala" and 21 <= case["line"] <= 164
    trace = P.run_kat(case, P.MmModel(case["replicas"], max_emit=2))
    assert trace and all(P.from_words(w).canonical() for t in trace for w in t)


def test_kats_cover_the_listed_specs():
    lines = [c["line"] for c in KATS]
    assert set(lines) == {21, 29, 34, 39, 55, 70, 101, 122, 141, 154, 160}
    assert all(lines.count(x) == 2 for x in (39, 55, 70, 101))  # merged both ways


# ------------------------------------------------------------------ the op rules
def test_add_binding_bumps_both_version_vectors():
    m = E().add_binding(3, 5, 2)
    assert m.keys.elements == {5: {3: 1}} and m.keys.vvector == {3: 1}
    assert m.values[5] == M.ORSet({2: {3: 1}}, {3: 1})
    m = m.add_binding(3, 5, 7).add_binding(3, 9, 2)
    assert m.keys.elements == {5: {3: 2}, 9: {3: 3}} and m.keys.vvector == {3: 3}    # the key's dots: the one birth dot
    assert m.values[5] == M.ORSet({2: {3: 1}, 7: {3: 2}}, {3: 2})                  # the set's own versions
    assert m.values[9] == M.ORSet({2: {3: 1}}, {3: 1})                             # a fresh set starts at zero
    other = m.add_binding(4, 5, 2)                                                # another node rebinds value 2
    assert other.values[5].elements[2] == {4: 1} and other.values[5].vvector == {3: 2, 4: 1}
    assert other.keys.elements[5] == {4: 1} and other.keys.vvector == {3: 3, 4: 1}


def test_remove_binding_keeps_the_set_version_and_may_take_the_key():
    m = E().add_binding(0, 1, 0).add_binding(0, 1, 1)
    r = m.remove_binding(0, 1, 0)
    assert r.entries == {1: frozenset({1})} and r.values[1].vvector == {0: 2}     # ORSet.remove: vvector untouched
    assert r.keys.elements == {1: {0: 3}} and r.keys.vvector == {0: 3}            # updated: keys.add
    gone = r.remove_binding(0, 1, 1)                                              # the set is left empty
    assert gone.entries == {} and gone.values == {} and gone.keys.elements == {}
    assert gone.keys.vvector == {0: 4}                                            # ... the + 1 of updated stays
    absent_key = E().remove_binding(2, 7, 3)
    assert absent_key.entries == {} and absent_key.keys.vvector == {2: 1} and absent_key.canonical()
    absent_value = m.remove_binding(0, 1, 5)                                      # an absent value of a live key
    assert absent_value.entries == m.entries and absent_value.keys.vvector == {0: 3} and absent_value.values[1] == m.values[1]
    absent_fresh = E().add_binding(0, 1, 0).remove(0, 1).remove_binding(0, 1, 4)  # an absent value of a fresh key
    assert absent_fresh.entries == {} and absent_fresh.keys.vvector == {0: 2}


def test_put_clears_then_adds_in_ascending_value_order():
    m = E().add_binding(1, 4, 6).add_binding(1, 4, 0)
    p = m.put(1, 4, [5, 2, 7])
    assert p.entries == {4: frozenset({2, 5, 7})}
    assert p.values[4] == M.ORSet({2: {1: 3}, 5: {1: 4}, 7: {1: 5}}, {1: 5})      # clear keeps the vvector; ascending
    assert p.keys.elements == {4: {1: 3}}
    empty = m.put(1, 4, [])
    assert empty.entries == {4: frozenset()} and empty.contains(4) and empty.size == 1   # a live key, an empty set
    assert empty.values[4] == M.ORSet({}, {1: 2}) and empty.canonical()
    full = E().put(0, 63, range(8))
    assert full.entries == {63: frozenset(range(8))} and full.values[63].vvector == {0: 8}
    assert P.apply_op(E(), 0, Op.put_set(63, range(8))) == full


def test_replace_binding():
    m = E().add_binding(0, 2, 1)
    assert m.replace_binding(0, 2, 1, 1) is m                                     # old == new returns `this`
    assert P.apply_op(m, 0, Op.replace_binding(2, 1, 1)) == m
    r = m.replace_binding(0, 2, 1, 3)
    assert r == m.add_binding(0, 2, 3).remove_binding(0, 2, 1)
    assert r.entries == {2: frozenset({3})} and r.keys.elements == {2: {0: 3}} and r.values[2].vvector == {0: 2}
    assert m.replace_binding(0, 2, 6, 3).entries == {2: frozenset({1, 3})}        # an absent old value


def test_remove_drops_the_set_and_leaves_the_version_vector():
    m = E().add_binding(0, 2, 1).add_binding(0, 3, 1)
    r = m.remove(0, 2)
    assert r.entries == {3: frozenset({1})} and r.keys.vvector == {0: 2} and r.canonical()
    assert not P.to_words(r).view(np.uint32)[2 * P.SET_WORD + 72 * 2:2 * P.SET_WORD + 72 * 3].any()


def test_unhandled_ops_and_version_range():
    for pay in (Op.make(Op.ADD, 512), Op.make(Op.REMOVE_BINDING, 512), Op.make(Op.PUT, 64 * 256), Op.make(Op.REPLACE_BINDING, 4096),
                Op.make(Op.REMOVE, 64), Op.make(Op.INCREMENT, 1), Op.make(Op.CLEAR), Op.make(Op.DELTA_TICK), Op.make(11, 0)):
        assert P.apply_op(E(), 0, pay) is None
    top = E(M.ORSet({1: {0: P.U32_MAX}}, {0: P.U32_MAX}), {1: M.ORSet({0: {0: 5}}, {0: 5})})
    with pytest.raises(P.VersionRange):
        P.apply_op(top, 0, Op.add_binding(2, 0))                                  # the key set's version
    assert P.apply_op(top, 0, Op.make(Op.REMOVE, 1)).entries == {}                # no updated, no bump
    assert P.apply_op(top, 0, Op.replace_binding(1, 3, 3)) == top
    top = E(M.ORSet({1: {0: 7}}, {0: 7}), {1: M.ORSet({0: {0: P.U32_MAX - 2}}, {0: P.U32_MAX - 2})})
    assert P.apply_op(top, 0, Op.put_set(1, [0, 1])).values[1].vvector == {0: P.U32_MAX}
    with pytest.raises(P.VersionRange):
        P.apply_op(top, 0, Op.put_set(1, [0, 1, 2]))                              # a value set's version


# ------------------------------------------------------------------ the anomalies, pinned
def test_concurrent_removal_from_a_set_is_lost():
    """"Note that on concurrent adds and removals for the same key (on the same set), removals can be lost"
    (DD/ORMultiMap.scala:65; ORMultiMapSpec "not handle concurrent updates to the same set"): the emptying
    removeBinding drops the key, so the other side's set is taken whole."""
    m = E().add_binding(0, 0, 0)
    m1, m2 = m.remove_binding(0, 0, 0), m.add_binding(1, 0, 1)
    assert m1.merge(m2).entries == {0: frozenset({0, 1})} and m2.merge(m1) == m1.merge(m2)
    kept = m.add_binding(0, 0, 2).remove_binding(0, 0, 0)                         # the key survives: the removal holds
    assert kept.merge(m2).entries == {0: frozenset({1, 2})}


def test_rebind_after_remove_gets_stale_dots_back():
    """A key removed and bound again starts a set with a zero version vector: it has forgotten that it saw, and
    removed, the old bindings, so a peer that still holds the old set gives their dots back -- value 1's dot 0 -> 2
    is newer than the fresh vector {0: 1} --, and the stale vector {0: 2} in turn covers the new binding's dot
    0 -> 1, which is dropped.  The order decides."""
    a = E().add_binding(0, 2, 0).add_binding(0, 2, 1)
    stale = a.copy()
    again = a.remove(0, 2).add_binding(0, 2, 5)
    assert again.entries == {2: frozenset({5})} and again.values[2] == M.ORSet({5: {0: 1}}, {0: 1})
    merged = again.merge(stale)
    assert merged.keys.elements == {2: {0: 3}}
    assert merged.entries == {2: frozenset({1})}          # value 1 is back, value 5 is gone, value 0 stays removed
    assert merged.values[2] == M.ORSet({1: {0: 2}}, {0: 2}) and stale.merge(again) == merged
    removed = a.remove(0, 2)
    assert stale.merge(removed).merge(again).entries == {2: frozenset({5})}       # ... and the order decides
    assert stale.merge(removed.merge(again)).entries == {2: frozenset({1})}
    peer = a.add_binding(1, 2, 3)                         # a peer of another node that bound a value of its own
    assert again.merge(peer).entries == {2: frozenset({1, 3})} and peer.merge(again) == again.merge(peer)


# ------------------------------------------------------------------ the join laws
def removal_free_pool(seed: int, n_ops: int = 260):
    """States of one history: 8 writers (one per node) bind, replace and unbind values and merge one another,
    sibling replicas copy and merge.  No key is ever removed: no `remove`, no `put`, and a removeBinding is issued
    only where it cannot empty the set -- each key holds a value that is never unbound or replaced (value 7, bound
    first).  Returns (pool, model): the same ops run through MmModel-style bookkeeping count the key removals."""
    rng = random.Random(seed)
    W = [E() for _ in range(P.NODES)]
    pool = [E()]
    removals = 0
    for i in range(1, n_ops + 1):
        k = rng.randrange(P.NODES)
        r = rng.random()
        key = rng.choice((0, 20, 31, 63, 8 + k))
        before = W[k]
        if key not in W[k].values:
            pay = Op.add_binding(key, 7)
        elif r < 0.40:
            pay = Op.add_binding(key, rng.randrange(7))
        elif r < 0.55:
            pay = Op.remove_binding(key, rng.randrange(7))
        elif r < 0.65:
            pay = Op.replace_binding(key, rng.randrange(7), rng.randrange(7))
        else:
            pay = None
        if pay is not None:
            W[k] = P.apply_op(W[k], k, pay)
            removals += sum(1 for x in before.values if x not in W[k].values)
        elif r < 0.88:
            W[k] = W[k].merge(W[rng.randrange(P.NODES)])
        else:
            pool.append(W[k].copy().merge(W[rng.randrange(P.NODES)]))
        assert W[k].canonical()
        if i % 5 == 0:
            pool.append(W[k].copy())
    return pool + [w.copy() for w in W], removals


def test_the_generator_stays_inside_the_cap():
    """Shown first, with the model: the histories of the join-law test drop no key."""
    for seed in (0x5EED, 11):
        pool, removals = removal_free_pool(seed)
        assert removals == 0
        assert all(7 in s.elements for m in pool for s in m.values.values())
        assert all(set(m.keys.elements) == set(m.values) for m in pool)


def test_merge_is_a_join_on_histories_without_key_removal():
    pool, removals = removal_free_pool(0x5EED)
    assert removals == 0 and len(pool) > 40 and max(len(m.values) for m in pool) >= 5
    assert max(len(s.elements) for m in pool for s in m.values.values()) >= 4
    rng = random.Random(7)
    for m in pool:
        assert m.merge(m) == m and m.canonical()
    for _ in range(500):
        a, b, c = rng.choice(pool), rng.choice(pool), rng.choice(pool)
        ab = a.merge(b)
        assert ab == b.merge(a)
        assert ab.merge(c) == a.merge(b.merge(c))
        assert ab.canonical()
        assert np.array_equal(P.to_words(P.from_words(P.to_words(ab))), P.to_words(ab))


# ------------------------------------------------------------------ words, ddata, Op, workload
def test_words_layout_and_canonical_form():
    m = E().add_binding(3, 5, 2).add_binding(3, 5, 7)
    w = P.to_words(m)
    u = w.view(np.uint32)
    base = 2 * 272 + 72 * 5
    assert u[5 * 8 + 3] == 2 and u[512 + 3] == 2 and not w[260:272].any()
    assert u[base + 3] == 2 and u[base + 8 + 8 * 2 + 3] == 1 and u[base + 8 + 8 * 7 + 3] == 2
    assert int(u[2 * 272:].astype(np.uint64).sum()) == 5 and base % 4 == 0
    assert P.from_words(w) == m and P.row_u32(m) == 32 + 4 + 72
    bad = w.copy()
    bad.view(np.uint32)[2 * 272 + 72 * 6] = 1  # a value-set word of a key without a live dot
    with pytest.raises(AssertionError):
        P.from_words(bad)


def test_ddata_words_round_trip():
    pool, _ = removal_free_pool(11)
    pool.append(E().put(2, 9, []).add_binding(2, 63, 7))
    for m in pool:
        w = P.to_words(m)
        d = ddata.ORMultiMap.from_words(w)
        assert d.entries == m.entries and d.size == m.size and d.is_empty == (m.size == 0)
        for k, s in m.values.items():
            assert d.contains(k) and d.get(k) == frozenset(s.elements) and d.get_or_else(k, frozenset({3})) == d.get(k)
            assert d.sets[k] == (s.vvector, s.elements) and d.dots[k] == m.keys.elements[k]
        assert d.get(40) is None and not d.contains(40) and d.get_or_else(40, frozenset({3})) == frozenset({3})
        assert d.vvector == m.keys.vvector and np.array_equal(d.to_words(), w)
    assert ddata.ORMultiMap.from_words(P.to_words(pool[-1])).entries == {9: frozenset(), 63: frozenset({7})}
    bad = P.to_words(pool[-1])
    bad.view(np.uint32)[2 * 272 + 72 * 10 + 9] = 5  # a value set without a live key dot
    with pytest.raises(ValueError):
        ddata.ORMultiMap.from_words(bad)
    bad = P.to_words(pool[-1])
    bad[265] = 1  # the padding
    with pytest.raises(ValueError):
        ddata.ORMultiMap.from_words(bad)
    with pytest.raises(ValueError):
        ddata.ORMultiMap.from_words(np.zeros(1296, np.uint64))


def test_op_encoding():
    assert Op.add_binding(63, 7) == (Op.ADD << 24) | 511 and Op.remove_binding(5, 2) == (9 << 24) | 5 | (2 << 6)
    assert Op.put_set(3, [0, 7]) == (Op.PUT << 24) | 3 | (0x81 << 6) and Op.put_set(0, []) == Op.PUT << 24
    assert Op.put_set(63, range(8)) == (8 << 24) | (64 * 256 - 1)
    assert Op.replace_binding(63, 7, 7) == (10 << 24) | 4095 and Op.replace_binding(1, 2, 3) == (10 << 24) | 1 | (2 << 6) | (3 << 9)
    for f, bad in ((Op.add_binding, [(64, 0), (-1, 0), (0, 8), (0, -1)]), (Op.remove_binding, [(64, 0), (0, 8)]),
                   (Op.put_set, [(64, []), (0, [8]), (0, [-1])]), (Op.replace_binding, [(64, 0, 1), (0, 8, 1), (0, 1, 8)])):
        for args in bad:
            with pytest.raises(ValueError):
                f(*args)
    assert CRDT_WORDS[Kind.ORMULTIMAP] == 2576 and Kind.ORMULTIMAP == 13
    assert not {Kind.ORMULTIMAP, Kind.PNCOUNTERMAP, Kind.LWWMAP} & set(CRDT_DELTA_WORDS)


def test_workload_builder():
    w = wl.crdt_ormultimap(96, rounds=4, fanout=2, binds_per_writer=16, removes=4, bucket_actors=32)
    assert w.n_actors == 96 and w.n_words == 2576 and w.max_emit == 3 and w.bucket_actors == 32
    assert w.ranges == [(0, 96, Kind.ORMULTIMAP, None)] and w.gossip == (2, wl.SEED) and w.lwwmap is None
    dst, src, pay = w.tells
    ops = pay[:8 * 20]
    assert (dst[:160] == np.repeat(np.arange(8), 20)).all() and (dst[160:] == np.arange(96)).all()
    code = ops >> 24
    assert (code == Op.REMOVE).sum() == 8 * 4 and (code == Op.ADD).sum() > (code == Op.REMOVE_BINDING).sum() > 0
    assert (code == Op.PUT).sum() > 0 and (code == Op.REPLACE_BINDING).sum() > 0
    assert all(P.apply_op(E(), 0, int(p)) is not None for p in ops)           # every argument in range
    assert (pay[160:] == Op.make(Op.GOSSIP, 3)).all() and (ops & 63).max() < 12
    assert wl.crdt_ormultimap(4).n_actors == 4 and len(wl.crdt_ormultimap(4).tells[0]) == 4 * 20 + 4
    assert np.array_equal(wl.ormultimap_ops(8, 16, 4), ops.reshape(8, 20))
    # the model runs it to quiescence and converges
    m = P.MmModel(**wl.crdt_ormultimap(24, rounds=12, bucket_actors=32).engine_kwargs())
    wl.crdt_ormultimap(24, rounds=12, bucket_actors=32).apply_to(m)
    st = m.run()
    assert st["in_flight"] == 0 and st["unhandled"] == 0 and m.converged() and len(m.maps[0].values) > 3
    assert m.key_removals > 0 and any(len(s.elements) > 1 for s in m.maps[0].values.values())
