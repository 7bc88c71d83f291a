"""Consistent-hashing and random routing without a GPU: the plain-Python hash, ring and model
(tests/router_model.py) against the reference spec's cases (tests/golden/router_kats.json restates
RoutingLogicSpec.scala:146-221), values worked by hand, and the properties consistent hashing exists for."""
import json
import pathlib
import re

import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import router_model as rm
from tests.router_model import ConsistentHashRing, RouterModel, concatenate_node_hash, murmur_string_hash

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "router_kats.json").read_text())
SPEC, DERIVED = KATS["spec"], KATS["self_derived"]
IDS = SPEC["routees"]


def messages():
    m = SPEC["messages"]
    return range(m["first"], m["last"] + 1), m["mapping_modulo"]


def verify_consistent_hashing(ring) -> dict:
    """verifyConsistentHashing (RoutingLogicSpec.scala:215-219): every message of a mapping group reaches one routee"""
    msgs, mod = messages()
    picked = {}
    for x in msgs:
        picked.setdefault(str(x % mod), set()).add(ring.node_for(str(x % mod)))
    assert all(len(v) == 1 for v in picked.values()), picked
    return {k: next(iter(v)) for k, v in picked.items()}


# ------------------------------------------------------------------ the spec's cases
@pytest.mark.parametrize("case", SPEC["hash_consistently"], ids=lambda c: f"factor{c['factor']}")
def test_hash_consistently(case):
    for names in case["sets"]:
        ring = ConsistentHashRing([IDS[x] for x in names], case["factor"])
        assert len(ring) == case["factor"] * len(names)
        assert set(verify_consistent_hashing(ring).values()) <= {IDS[x] for x in names}


@pytest.mark.parametrize("which", ["several_removed", "several_added"])
def test_hash_consistently_when_several_change(which):
    case = SPEC[which]
    picks = [verify_consistent_hashing(ConsistentHashRing([IDS[x] for x in names], case["factor"])) for names in case["sets"]]
    small, large = sorted(picks, key=lambda p: len(set(p.values())))
    kept = {IDS[x] for x in min(case["sets"], key=len)}
    for k, node in large.items():  # a key that a surviving routee owned on the larger ring stays with it
        if node in kept:
            assert small[k] == node, (k, node, small[k])


def test_no_routees_is_an_error():
    case = SPEC["no_routees"]
    with pytest.raises(LookupError) as e:
        ConsistentHashRing((), case["factor"]).node_for(str(case["message"]))
    assert re.fullmatch(case["error_regex"], str(e.value))


def test_a_factor_below_one_is_refused():
    case = SPEC["factor_zero"]
    with pytest.raises(typed.CompileError) as e:
        typed.Routers.group(typed.ServiceKey("w")).with_consistent_hash_routing(case["factor"], lambda m: m.arg)
    assert str(e.value) == case["error"]
    with pytest.raises(ValueError):
        ConsistentHashRing((1, 2), case["factor"])


# ------------------------------------------------------------------ drift: the values the model computed when written
def test_self_derived_values():
    for s, h in DERIVED["string_hash"].items():
        assert murmur_string_hash(s) == h, s
    for p in DERIVED["ring_point"]:
        assert concatenate_node_hash(murmur_string_hash(str(p["id"])), p["vnode"]) == p["hash"], p


# ------------------------------------------------------------------ wrapping arithmetic, worked by hand
def test_wrapping_arithmetic_by_hand():
    # "": no character; startHash(0 * seedString) = 0 ^ visibleMagic = 0x971e137b, then finalizeHash alone
    assert rm.finalize_hash(0x971e137b) == 0x9eb43457 == murmur_string_hash("")
    # "0" (odd length 1): startHash(1 * 0xf7ca7fd2) = 0xf7ca7fd2 ^ 0x971e137b = 0x60d46ca9; one extendHash with the lone
    # character 0x30 and the first magics; the products wrap mod 2^32
    assert 0xf7ca7fd2 ^ 0x971e137b == 0x60d46ca9
    assert rm.extend_hash(0x60d46ca9, 0x30, 0x95543787, 0x2ad7eb25) == 0xf58a1e86
    assert rm.finalize_hash(0xf58a1e86) == 0x7f9a45f7 == murmur_string_hash("0")
    # "10" (even length 2): startHash(2 * 0xf7ca7fd2 mod 2^32 = 0xef94ffa4) = 0x788aecdf; one extendHash with
    # ('1' << 16) + '0' = 0x00310030; no odd tail
    assert (2 * 0xf7ca7fd2) & 0xFFFFFFFF == 0xef94ffa4 and 0xef94ffa4 ^ 0x971e137b == 0x788aecdf
    assert rm.extend_hash(0x788aecdf, 0x00310030, 0x95543787, 0x2ad7eb25) == 0x15a89c5b
    assert rm.finalize_hash(0x15a89c5b) == 0x283cd7a6 == murmur_string_hash("10")
    # "123" (odd length 3): the second step uses nextMagicA / nextMagicB = magic * 5 + mixer, wrapping
    assert (0x95543787 * 5 + 0x7b7d159c) & 0xFFFFFFFF == 0x66222b3f and (0x2ad7eb25 * 5 + 0x6bce6396) & 0xFFFFFFFF == 0x4205fb4f
    assert rm.extend_hash(0xadd8e656, 0x33, 0x66222b3f, 0x4205fb4f) == 0x5df0c10d
    assert murmur_string_hash("123") == 0xbffd6d2b
    # extendHash's rotate: value * magicA = 0x80000001 rotated left by 11 is 0x00000C00
    assert rm._rotl(0x80000001, 11) == 0x00000C00


# ------------------------------------------------------------------ the ring's order
def test_signed_ordering_wraps_to_entry_zero():
    ring = ConsistentHashRing.from_entries([(0x7FFFFFF0, 1), (-0x80000000, 2), (-5, 3), (10, 4)])
    assert [a for _, a in ring.entries] == [2, 3, 4, 1]  # negative hashes first: signed, not unsigned, order
    assert ring.node_for_hash(-0x80000000) == 2 and ring.node_for_hash(-6) == 3 and ring.node_for_hash(-4) == 4
    assert ring.node_for_hash(11) == 1 and ring.node_for_hash(0x7FFFFFF0) == 1
    assert ring.node_for_hash(0x7FFFFFF1) == 2  # past the last entry: entry 0
    assert ring.hashes_u32().tolist() == [0x80000000, 0xFFFFFFFB, 10, 0x7FFFFFF0]
    real = ConsistentHashRing(range(50), 5)
    hs = [h for h, _ in real.entries]
    assert hs == sorted(hs) and hs[0] < 0 < hs[-1]


def test_the_collision_rule():
    ring = ConsistentHashRing.from_entries([(7, 9), (7, 4), (7, 6), (100, 1)])
    assert ring.entries[:3] == [(7, 4), (7, 6), (7, 9)]
    assert ring.node_for_hash(7) == 4 and ring.node_for_hash(-1) == 4 and ring.node_for_hash(8) == 1


# ------------------------------------------------------------------ what consistent hashing is for
def test_one_node_leaving_or_joining_moves_only_its_keys():
    nodes, factor, keys = list(range(100, 150)), 5, range(1 << 12)
    full = ConsistentHashRing(nodes, factor)
    owner = {x: full.node_for(str(x)) for x in keys}
    assert len(set(owner.values())) > 40
    for gone in (100, 123, 149):
        less = ConsistentHashRing([a for a in nodes if a != gone], factor)
        for x in keys:
            got = less.node_for(str(x))
            if owner[x] != gone:
                assert got == owner[x], (gone, x)  # a key of another node stays
            else:
                assert got != gone
        # ... and adding `gone` back moves keys only to it
        for x in keys:
            assert owner[x] in (less.node_for(str(x)), gone)
    modulo_moved = sum(1 for x in keys if nodes[x % 50] != [a for a in nodes if a != 100][x % 49])
    hashed_moved = sum(1 for x in keys if owner[x] == 100)
    assert hashed_moved < len(keys) // 10 < modulo_moved  # (the modulo stand-in moves almost every key)


# ------------------------------------------------------------------ random routing
def test_random_index_is_in_range_and_repeatable():
    for size in (1, 2, 7, 64, 1000):
        idx = [rm.random_index(5, 3, c, size) for c in range(200)]
        assert all(0 <= i < size for i in idx)
        assert idx == [rm.random_index(5, 3, c, size) for c in range(200)]
        if size > 1:
            assert len(set(idx)) > 1
    assert rm.random_index(5, 3, 0x01000007, 64) == rm.random_index(5, 3, 7, 64)  # (the counter's low 24 bits)
    assert [rm.random_index(5, 3, c, 64) for c in range(50)] != [rm.random_index(6, 3, c, 64) for c in range(50)]
    assert [rm.random_index(5, 3, c, 64) for c in range(50)] != [rm.random_index(5, 4, c, 64) for c in range(50)]


def _model(w):
    m = RouterModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def test_the_counter_advances_only_on_a_hit():
    w = wl.random_pool(n_routers=4, n_workers=8, ticks=8, quota=1, seed=9)  # every worker stops after one job
    m = _model(w)
    w.run_schedule(m)
    words, alive = m.read_state()
    info, rinfo = m.receptionist_info(), m.router_info()
    assert info["routed"] == rinfo["random"] == int(words[:4, 0].sum())  # the counters moved once per hit
    assert info["routed"] + info["no_routees"] == 32 == int(words[:4, 1].sum())
    assert info["no_routees"] > 0 and rinfo["hashed"] == 0 and rinfo["ring_size"] == [0] * 8


def test_sticky_sessions_on_the_model():
    w = wl.sticky_sessions(n_clients=64, n_routers=4, n_workers=16, n_spare=4, quota=0, virtual_nodes_factor=3, ticks=6,
                           join_at=2, seed=2)
    m = _model(w)
    assert m.router_info()["ring_size"][0] == 12 * 3 and m.router_info()["ring_rebuilds"] == 0
    st = w.run_schedule(m)
    rinfo = m.router_info()
    assert rinfo["ring_size"][0] == 16 * 3 and rinfo["ring_rebuilds"] == 1 and rinfo["hashed"] == 64 * 6
    assert st["in_flight"] == 0 and st["dead_letters"] == 0
    hs, ids = m.read_hash_ring(0)
    assert len(hs) == 48 and sorted(set(ids.tolist())) == list(range(68, 84))
    signed = hs.astype(np.int64) - ((hs.astype(np.int64) >> 31) << 32)
    assert (np.diff(signed) >= 0).all()
    # the last session a worker served is one of those the final ring gives it
    words, _ = m.read_state()
    ring = ConsistentHashRing(range(68, 84), 3)
    mine = {}
    for c in range(64):
        mine.setdefault(ring.node_for(str(int(words[c, 0]))), set()).add(int(words[c, 0]))
    assert len(mine) > 4
    for a, sessions in mine.items():
        assert int(words[a, 1]) in sessions, a
