"""TEST INFRASTRUCTURE ONLY.  Crafted CRDT states for the kernels that merge them.

The seeded workloads (workloads.crdt_ops on states that start at zero) never fill a snapshot row,
never populate all 64 lanes of the wave and never pass version 15 (DESIGN.md §8 "crafted CRDT
states").  This module makes ORSet replicas that do, and that are still *reachable*: every state is
produced by the model (tests/crdt_model.py) from one history of 8 writer nodes -- adds on a node's
own lineage, removes, clears, merges and copies of sibling replicas -- so that every dot (node,
version) is born once.  The versions are then rescaled per node by a strictly monotone map, which
keeps every order relation a merge looks at, hence reachability: the reference draws versions from
a JVM-wide counter (DD/VersionVector.scala:76-80), so gaps between a node's versions are ordinary.

Reachability is what makes ORSet.merge a join (commutative, associative, idempotent) on these
states, and that is what lets a GPU test compute an expected state from the set of predicted senders
without knowing their arrival order (tests/test_crdt_model.py checks the join laws on every state
made here).
"""
from __future__ import annotations

import functools
import random

import numpy as np

from akka_amd import workloads as wl
from akka_amd.engine import CRDT_DELTA_WORDS, CRDT_WORDS, Kind, NO_SENDER, Op
from tests import crdt_model as M
from tests.prio_model import fanout_rand

NODES, ELEMS = M.NODES, M.ELEMS
U32_MAX = (1 << 32) - 1
U64_MAX = (1 << 64) - 1
# the version steps that must come out of the rescaling (16-bit, sign-bit and wrap neighbourhoods)
SPECIAL_VERSIONS = (65535, 65536, 65537, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1)

# Per node: [(from_version, base)]: versions below the first `from` stay as they are (small), a version
# v >= from maps to base + (v - from) up to the next break.  from < 0 counts from the node's last
# version (-2: the last two).  Every node's history has at least 64 versions (phase A below).
SCALES = {
    0: [],                                                       # small throughout
    1: [(14, 65535)],                                            # 65535, 65536, 65537, ...
    2: [(33, 2**31 - 1)],                                        # 2^31 - 1, 2^31, 2^31 + 1, ...
    3: [(-2, 2**32 - 2)],                                        # the last two: 2^32 - 2, 2^32 - 1
    4: [(9, 65535), (40, 2**31 - 1)],
    5: [(5, 65535), (50, 2**31 - 1), (-2, 2**32 - 2)],
    6: [(64, 2**31 - 1)],
    7: [(2, 2**31 - 1)],                                         # all but one version >= 2^31 - 1
}
# for the version-wrap scenario: node 3's last version is 2^32 - 2, so its writer has one add left
WRAP_SCALES = dict(SCALES)
WRAP_SCALES[3] = [(20, 2**31 + 5), (-1, 2**32 - 2)]
# for replicas that take a few more adds in the test: every node's last version leaves room for 13 adds
OPS_SCALES = {n: [(f, b - 14 if b == 2**32 - 2 else b) for f, b in br] for n, br in SCALES.items()}
VARIANTS = {"edge": SCALES, "wrap": WRAP_SCALES, "ops": OPS_SCALES}


def _scale_fn(breaks, vmax):
    br = sorted((f if f >= 0 else vmax + 1 + f, b) for f, b in breaks)
    for (f0, b0), (f1, b1) in zip(br, br[1:]):
        assert f0 < f1 and b0 + (f1 - 1 - f0) < b1, "the version map must be strictly monotone"
    if br:
        assert br[0][0] >= 1 and br[0][0] - 1 < br[0][1] and br[-1][1] + (vmax - br[-1][0]) <= U32_MAX

    def f(v):
        out = v
        for fr, base in br:
            if v >= fr:
                out = base + (v - fr)
        return out
    return f


def rescale(states, scales):
    """The same strictly monotone map per node over every dot and version-vector entry of `states`."""
    vmax = {n: max([s.vvector.get(n, 0) for s in states] + [0]) for n in range(NODES)}
    fn = {n: _scale_fn(scales.get(n, []), vmax[n]) for n in range(NODES)}
    out = []
    for s in states:
        out.append(M.ORSet({e: {n: fn[n](v) for n, v in d.items()} for e, d in s.elements.items()},
                           {n: fn[n](v) for n, v in s.vvector.items()}))
    return out


def _history(seed):
    """One history of 8 writer nodes; the named snapshots, in a fixed order (versions unscaled)."""
    rng = random.Random(seed)
    snaps = []

    def snap(name, s):
        snaps.append((name, s.copy()))

    snap("empty", M.ORSet())
    # phase A: every node adds every element on its own, then all merge -> 512 live dots
    W = [M.ORSet() for _ in range(NODES)]
    w7_short = None
    for k in range(NODES):
        order = list(range(ELEMS))
        rng.shuffle(order)
        for i, e in enumerate(order):
            if k == 7 and i == ELEMS - 1:
                w7_short = W[7].copy()
            W[k] = W[k].add(k, e)
            if k == 0 and i == 0:
                snap("single_dot", W[0])
    snap("writer1", W[1])  # 64 dots of one node; writer1 / writer2 are Concurrent
    snap("writer2", W[2])
    full = M.merge_all(W)
    snap("full512", full)
    snap("full511", M.merge_all(W[:7] + [w7_short]))  # Before full512: one dot short
    s = full
    for e in range(ELEMS - 1):
        s = s.remove(e)
    snap("only63", s)  # Same vvector as full512, one element of 8 dots
    s = full
    for e in range(48):
        s = s.remove(e)
    snap("high16", s)  # populated elements exactly 48..63
    # phase B: the writers go on from the full set; adds and removes touch a few elements only, so most
    # elements keep their 8 dots
    W = [full.copy() for _ in range(NODES)]
    hot = [0, 1, 2, 3, 31, 32, 62, 63]
    for k in (3, 5):  # (the nodes whose last two versions are scaled to 2^32 - 2, 2^32 - 1 have later adds)
        W[k] = W[k].add(k, hot[k])
    for step in range(56):
        k = rng.randrange(NODES)
        r = rng.random()
        if r < 0.40:
            W[k] = W[k].add(k, rng.choice(hot))
        elif r < 0.55:
            W[k] = W[k].remove(rng.choice(hot))
        elif r < 0.80:
            W[k] = W[k].merge(W[rng.randrange(NODES)])
        else:  # a sibling replica (never adds): a copy that removes a few elements and merges a neighbour
            s = W[k].copy()
            for e in rng.sample(range(ELEMS), 3):
                s = s.remove(e)
            if rng.random() < 0.5:
                s = s.merge(W[rng.randrange(NODES)])
            snap(f"sibling_{step}", s)
        if step % 7 == 6:
            snap(f"node{k}_step{step}", W[k])
    for k in (3, 5):
        W[k] = W[k].add(k, hot[k + 1])
    snap("cleared", W[6].clear())  # no elements, the history kept: its vvector makes seen dots vanish
    for k in range(NODES):
        snap(f"node{k}_last", W[k])
    return snaps


@functools.lru_cache(maxsize=None)
def _pool(seed, variant):
    snaps = _history(seed)
    states = rescale([s for _, s in snaps], VARIANTS[variant])
    return tuple((name, st) for (name, _), st in zip(snaps, states))


def pool(seed: int = 0x5EED, variant: str = "edge") -> dict:
    """{name: ORSet} of the crafted, rescaled snapshots (copies: callers may keep them).  variant: "edge"
    (SCALES: versions up to 2^32 - 1), "wrap" (node 3's writer has one add left) or "ops" (every node has
    room for 13 more adds)."""
    return {name: s.copy() for name, s in _pool(seed, variant)}


def population(n: int, seed: int = 0x5EED, variant: str = "edge") -> list:
    """n replicas: the pool in order (so every dial is present once n >= len(pool)), then seeded
    repeats of pool states (a repeat and its original are Same)."""
    p = [s for _, s in _pool(seed, variant)]
    rng = random.Random(seed ^ 0xC0FFEE)
    out = [p[i].copy() if i < len(p) else rng.choice(p).copy() for i in range(n)]
    return out


def census(states) -> dict:
    """The quantities of DESIGN.md §8's census table over ORSet states."""
    live = [sum(len(d) for d in s.elements.values()) for s in states]
    versions = [v for s in states for d in s.elements.values() for v in d.values()] + \
               [v for s in states for v in s.vvector.values()]
    return {
        "max_live_dots": max(live, default=0),
        "max_populated_elements": max((len(s.elements) for s in states), default=0),
        "max_dots_per_element": max((len(d) for s in states for d in s.elements.values()), default=0),
        "max_version": max(versions, default=0),
        "elements_populated_somewhere": len({e for s in states for e in s.elements}),
    }


def assert_census(states):
    """What every crafted-state test asserts of its own inputs, so that a later edit cannot quietly
    shrink the cases."""
    c = census(states)
    assert c["max_live_dots"] == 512, c
    assert c["max_dots_per_element"] == 8, c
    assert c["elements_populated_somewhere"] == 64, c
    assert c["max_version"] >= 2**31, c
    return c


def versions_used(states) -> set:
    return {v for s in states for d in s.elements.values() for v in d.values()} | \
           {v for s in states for v in s.vvector.values()}


def pair_census(states, pairs) -> dict:
    """Over (sender, receiver) index pairs: how many of each VersionVector relation (sender compared to
    receiver), how many receiver elements absent at the sender vanish (every dot dominated by the
    sender's vvector) and how many stay."""
    out = {"==": 0, "<": 0, ">": 0, "<>": 0, "vanish": 0, "stay": 0}
    for s, r in pairs:
        a, b = states[s], states[r]
        out[M.vv_compare(a.vvector, b.vvector)] += 1
        for e, dot in b.elements.items():
            if e not in a.elements:
                out["vanish" if not M.subtract_dots(dot, a.vvector) else "stay"] += 1
    return out


# ------------------------------------------------------------------ peers
GOSSIP_TAG = 0x08000000


def crdt_peer(seed: int, self_id: int, round_: int, j: int, n: int) -> int:
    """crdt_peer (oracle/crdt_ref.h, akka_amd/csrc/agx_crdt.h): uniform over the other n - 1 actors."""
    d = fanout_rand(seed, self_id, round_ | GOSSIP_TAG, j) % (n - 1)
    return d + 1 if d >= self_id else d


def crdt_key_peer(seed: int, self_id: int, round_: int, j: int, n: int) -> int:
    """crdt_key_peer: delta-CRDT mode, uniform over the other replicas of the key [g, g + m)."""
    g = self_id & ~(NODES - 1)
    m = min(NODES, n - g)
    node = self_id % NODES
    d = fanout_rand(seed, self_id, round_ | GOSSIP_TAG, j) % (m - 1)
    return self_id - node + (d + 1 if d >= node else d)


def senders(n: int, seed: int, fanout: int, round_: int, delta: bool, ticking=None) -> dict:
    """{receiver: [senders]} of one GossipTick at countdown `round_` by every actor in `ticking`
    (default: all n)."""
    out = {r: [] for r in range(n)}
    for s in (range(n) if ticking is None else ticking):
        if delta and min(NODES, n - (s & ~(NODES - 1))) < 2:
            continue
        for j in range(fanout):
            out[(crdt_key_peer if delta else crdt_peer)(seed, s, round_, j, n)].append(s)
    return out


def seed_for(sender: int, receiver: int, n: int, delta: bool = False) -> int:
    """A gossip seed under which `sender`'s one gossip at countdown 0 goes to `receiver`."""
    for seed in range(1, 4096):
        if (crdt_key_peer if delta else crdt_peer)(seed, sender, 0, 0, n) == receiver:
            return seed
    raise AssertionError("no seed found")


# ------------------------------------------------------------------ counters
def counter_population(kind: int, n: int, seed: int = 0x5EED) -> np.ndarray:
    """(n, 8 | 16) u64 counter states whose slots differ in both u32 halves: a palette around 2^32 and
    2^64, pairs with a.lo > b.lo and a.hi < b.hi, and seeded 64-bit values.  Any counter states join
    (slot-wise max is a lattice on all of them); for a PNCounter both halves are drawn independently."""
    rng = random.Random(seed ^ (kind << 20))
    palette = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, U64_MAX, U64_MAX - 1, (5 << 32) | 7, (4 << 32) | 0xFFFFFFF0,
               1 << 63, (1 << 63) - 1, (1 << 31), (0xFFFFFFFF << 32), 0x00000001FFFFFFFF, 0x0000000200000000]
    W = CRDT_WORDS[kind]
    out = np.zeros((n, W), np.uint64)
    for a in range(n):
        for w in range(W):
            out[a, w] = rng.choice(palette) if rng.random() < 0.7 else rng.getrandbits(64)
    return out


def counter_census(words: np.ndarray, pairs) -> dict:
    """Over (sender, receiver) pairs and slots: how many slot pairs cross (a.lo > b.lo and a.hi < b.hi),
    and which of the edge values occur."""
    lo, hi = words & np.uint64(0xFFFFFFFF), words >> np.uint64(32)
    cross = 0
    for s, r in pairs:
        cross += int(((lo[s] > lo[r]) & (hi[s] < hi[r])).sum())
    vals = set(int(x) for x in np.unique(words))
    return {"cross": cross, "edges": {v for v in (0, 2**32 - 1, 2**32, U64_MAX) if v in vals}}


def assert_counter_census(words, pairs):
    c = counter_census(words, pairs)
    assert c["cross"] > 0 and c["edges"] == {0, 2**32 - 1, 2**32, U64_MAX}, c
    return c


# ------------------------------------------------------------------ engine shapes
SHAPES = ("or_only", "mixed", "delta_gossip")
N_BESIDE = 8  # replicas of the other data type in the `mixed` shape


def orset_words(states) -> np.ndarray:
    return np.stack([M.orset_to_words(s) for s in states]) if len(states) else np.zeros((0, M.ORSET_WORDS), np.uint64)


def workload(ranges, tells, *, delta: bool = False, fanout: int = 2, seed: int = 1, throughput: int = 5,
             capacity: int = 0, bucket_actors: int = 32, name: str = "crafted") -> wl.Workload:
    """An engine of consecutive CRDT ranges [(kind, (count, words) u64 initial states)] with host tells
    (dst, payload) in order; `delta`: delta-CRDT replication on (no DeltaPropagationTick is told, so
    only full-state gossip within the keys of 8 runs)."""
    widths = CRDT_DELTA_WORDS if delta else CRDT_WORDS
    W = max(widths[k] for k, _ in ranges)
    rs, first = [], 0
    for kind, words in ranges:
        words = np.ascontiguousarray(np.asarray(words, np.uint64))
        rs.append((first, len(words), kind, words))
        first += len(words)
    dst = np.asarray(tells[0], np.uint32)
    pay = np.asarray(tells[1], np.uint32)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return wl.Workload(name, first, W, max(4, fanout + 1) if delta else fanout + 1, throughput, capacity, rs,
                       gossip=(fanout, seed), delta_crdt=50 if delta else 0, tells=(dst, src, pay),
                       bucket_actors=bucket_actors)


def orset_shape(shape: str, words: np.ndarray, tells, **kw) -> wl.Workload:
    """The ORSet replicas `words` in one of the three engine shapes, each of which reaches another merge
    implementation: or_only (the wave path, sparse rows), mixed (a trailing range of GCounter replicas:
    crdt_apply, dense rows) and delta_gossip (delta-CRDT on: dense rows plus deltaVersions, keys of 8)."""
    assert shape in SHAPES
    ranges = [(Kind.ORSET, words)]
    if shape == "mixed":
        ranges.append((Kind.GCOUNTER, counter_population(Kind.GCOUNTER, N_BESIDE)))
    return workload(ranges, tells, delta=shape == "delta_gossip", name=f"crafted_{shape}", **kw)


def tells_in_order(per_actor: dict):
    """Host tells {actor: [payloads in order]} as (dst, payload) arrays; the tells of one actor keep
    their order (the staged batch is delivered in staging order per destination)."""
    dst, pay = [], []
    for a in sorted(per_actor):
        for p in per_actor[a]:
            dst.append(a)
            pay.append(p)
    return np.array(dst, np.uint32), np.array(pay, np.uint32)


def gossip(arg: int = 0) -> int:
    return Op.make(Op.GOSSIP, arg)
