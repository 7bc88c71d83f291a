"""Deterministic synthetic workloads (BASELINE.json configs C1..C5).

Everything is integer and seeded (SplitMix64 counter RNG),
so the same inputs feed the GPU engine, the CPU oracles and the benchmark.
A workload is a plain description: actor ranges + behaviour params + initial
tells; `apply_to(target)` installs it into anything with the engine's
register_range / set_* / tell interface.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .engine import CRDT_DELTA_WORDS, CRDT_NODES, CRDT_WORDS, DELTA_WRITE, LWWMAP_DELTA_WORDS, Kind, NO_SENDER, Op

SEED = 0x5EED
M64 = (1 << 64) - 1


def splitmix64_np(x: np.ndarray) -> np.ndarray:
    """Vectorised SplitMix64 finaliser (uint64 wrapping arithmetic)."""
    z = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


@dataclass
class Workload:
    name: str
    n_actors: int
    n_words: int
    max_emit: int
    throughput: int
    capacity: int
    ranges: list = field(default_factory=list)  # (first, count, kind, init_state or None)
    ring_stride: int | None = None
    gossip: tuple | None = None  # (fanout, seed)
    delta_crdt: int = 0          # Replicator max-delta-size (0 = full-state gossip only)
    lwwmap: tuple | None = None  # (clock, base) of an LWWMap engine (agx_set_lwwmap)
    lwwmap_delta: int = 0        # max-delta-size of an LWWMap engine with delta replication (agx_set_lwwmap_delta; 0 = off)
    behaviors: object = None     # compiled behaviour tables (akka_amd.typed.Tables)
    fanout: tuple | None = None  # (k, seed, cdf, perm)
    graph: tuple | None = None   # (row_ptr, col)
    tells: tuple | None = None   # (dst, src, payload)
    bucket_actors: int = 0       # GPU engine hint (agx_cfg.bucket_actors): deep mailboxes want small buckets
    mailbox_classes: dict = field(default_factory=dict)  # class -> capacity (agx_set_mailbox_class)
    mailboxes: list = field(default_factory=list)         # (first, count, class) (agx_set_mailbox)
    outbound: tuple | None = None                         # (first_host_id, n_host) (agx_set_outbound)
    # class -> 256 priorities by message tag, bytes or a sequence (agx_set_mailbox_priority)
    mailbox_priorities: dict = field(default_factory=dict)
    stash: dict = field(default_factory=dict)  # class -> stash capacity (agx_set_stash: a deque-based mailbox)
    # timers (agx_set_timers / agx_start_timers): {"n_keys": k, "starts": [(first, count, key, periodic, delay,
    # delays or None, payload)], "receive_timeout": {"transparent": message tags, "starts": [(first, count, delay,
    # payload)]}} -- empty: no timers; without "receive_timeout": no receive timeouts (agx_set_receive_timeout /
    # agx_start_receive_timeout, on top of the timers: behaviours that use only a receive timeout pass n_keys 1);
    # "ask": True -- the ask pattern (agx_set_ask, on top of the timers; not together with "receive_timeout");
    # "receive_timeout" may hold "sharding": the entity types (agx_set_sharding, typed.Tables.entity_types)
    timers: dict = field(default_factory=dict)
    # death watch (agx_set_death_watch / agx_start_watch): {"n_slots": k, "starts": [(first, count, watchees or
    # None, offset, message or None)]} -- empty: no death watch
    watch: dict = field(default_factory=dict)
    # supervision (agx_set_supervision): {"rows": per compiled behaviour its supervisor entries, inner first
    # (typed.Tables.supervisors), "backoff": per compiled behaviour a backoff row per entry (agx_set_backoff, on top;
    # typed.Tables.backoff; absent or empty: plain restarts)} -- empty: no supervision
    supervision: dict = field(default_factory=dict)
    # children (agx_set_children / agx_spawn_children, on top of `watch`): {"regions": [(first_parent, n_parents,
    # first_child, max_children)], "sites": typed.Tables.spawn_sites, "spawns": [(first, count, site, arg)]} --
    # empty: no children
    children: dict = field(default_factory=dict)
    # the receptionist (agx_set_receptionist / agx_register_services): {"n_keys": k, "capacity": ids per listing,
    # "starts": [(first, count, key)]} -- empty: no receptionist
    receptionist: dict = field(default_factory=dict)
    # pub-sub topics (agx_set_topics, on top of `receptionist`): {"log_capacity": publications per tick} -- empty: no
    # topics
    topics: dict = field(default_factory=dict)
    # Subscribe / Listing (agx_set_listings / agx_subscribe_listings, on top of `topics`): {"payloads": the Listing
    # payload per key (typed.Tables.listing_payloads), "starts": [(first, count, key)]} -- empty: no listings
    listings: dict = field(default_factory=dict)
    # consistent-hashing and random routing (agx_set_router_logics, on top of `receptionist`, not with `topics`):
    # {"hashed_keys_mask": m, "virtual_nodes_factor": f, "seed": s} -- empty: no router logics
    router_logics: dict = field(default_factory=dict)
    # host tells that follow the clock: schedule[t] = (dst, src, payload) is staged before tick t + 1 (run_schedule)
    schedule: list = field(default_factory=list)

    def engine_kwargs(self) -> dict:
        """Semantic parameters (shared by the GPU engine and the CPU oracles)."""
        return dict(n_actors=self.n_actors, throughput=self.throughput, capacity=self.capacity,
                    n_words=self.n_words, max_emit=self.max_emit)

    def gpu_kwargs(self) -> dict:
        """engine_kwargs + the GPU engine's layout hints (EngineConfig)."""
        return dict(self.engine_kwargs(), bucket_actors=self.bucket_actors)

    def apply_to(self, target, stage_tells: bool = True) -> None:
        for first, count, kind, init in self.ranges:
            target.register_range(first, count, kind, init)
        for cls, cap in self.mailbox_classes.items():
            target.set_mailbox_class(cls, cap)
        for first, count, cls in self.mailboxes:
            target.set_mailbox(first, count, cls)
        for cls, table in self.mailbox_priorities.items():  # (empty: targets without the call are unaffected)
            target.set_mailbox_priority(cls, table)
        for cls, cap in self.stash.items():  # (empty: targets without the call are unaffected)
            target.set_stash(cls, cap)
        if self.outbound is not None:
            target.set_outbound(*self.outbound)
        if self.ring_stride is not None:
            target.set_ring(self.ring_stride)
        if self.gossip is not None:
            target.set_gossip(*self.gossip)
        if self.delta_crdt:
            target.set_delta_crdt(self.delta_crdt)
        if self.lwwmap is not None:
            target.set_lwwmap(*self.lwwmap)
        if self.lwwmap_delta:
            target.set_lwwmap_delta(self.lwwmap_delta)
        if self.behaviors is not None:
            target.set_behaviors(self.behaviors)
        if self.receptionist:  # (empty: targets without the calls are unaffected)
            target.set_receptionist(self.receptionist["n_keys"], self.receptionist["capacity"])
            for first, count, key in self.receptionist.get("starts", ()):
                target.register_services(first, count, key)
        if self.router_logics:  # (empty: targets without the call are unaffected)
            target.set_router_logics(self.router_logics["hashed_keys_mask"], self.router_logics.get("virtual_nodes_factor", 0),
                                     self.router_logics.get("seed", 0))
        if self.topics:  # (empty: targets without the call are unaffected)
            target.set_topics(self.topics["log_capacity"])
        if self.listings:  # (empty: targets without the calls are unaffected)
            target.set_listings(self.listings["payloads"])
            for first, count, key in self.listings.get("starts", ()):
                target.subscribe_listings(first, count, key)
        if self.timers:  # (empty: targets without the calls are unaffected)
            target.set_timers(self.timers["n_keys"])
            if self.timers.get("ask"):  # (the ask pattern, on top of the timers: agx_set_ask)
                target.set_ask()
            for first, count, key, periodic, delay, delays, payload in self.timers.get("starts", ()):
                target.start_timers(first, count, key, delay, periodic=periodic, delays=delays, payload=payload)
            rt = self.timers.get("receive_timeout")
            if rt is not None:
                target.set_receive_timeout(rt.get("transparent", ()))
                for first, count, delay, payload in rt.get("starts", ()):
                    target.start_receive_timeout(first, count, delay, payload)
                if rt.get("sharding"):  # (sharded entities, on top of the receive timeouts: agx_set_sharding)
                    target.set_sharding(rt["sharding"])
        if self.watch:  # (empty: targets without the calls are unaffected)
            target.set_death_watch(self.watch["n_slots"])
            if self.children:  # (before the setup watches: a child block's ids are "not created yet", not "dead")
                target.set_children(self.children["regions"], self.children["sites"])
            for first, count, watchees, offset, message in self.watch.get("starts", ()):
                target.start_watch(first, count, watchees, offset=offset, message=message)
        if self.supervision:  # (empty: targets without the call are unaffected)
            target.set_supervision(self.supervision["rows"])
            if self.supervision.get("backoff"):  # (restartWithBackoff, on top of supervision: agx_set_backoff)
                target.set_backoff(self.supervision["backoff"])
        if self.children:  # (empty: targets without the calls are unaffected; set_children: with the watch above)
            for first, count, site, arg in self.children.get("spawns", ()):
                target.spawn_children(first, count, site, arg)
        if self.fanout is not None:
            target.set_fanout(*self.fanout)
        if self.graph is not None:
            if len(self.graph) == 3 and isinstance(self.graph[0], str):  # ("rmat", row_ptr, params)
                _, row, prm = self.graph
                if hasattr(target, "set_graph_rmat"):
                    target.set_graph_rmat(row, *prm)
                else:
                    target.set_graph(row, rmat_cols(int(row[-1]), self.n_actors, *prm))
            else:
                target.set_graph(*self.graph)
        if stage_tells and self.tells is not None:
            dst, src, pay = self.tells
            target.tell(dst, pay, src)

    @property
    def n_tells(self) -> int:
        return 0 if self.tells is None else int(len(self.tells[0]))

    def run_schedule(self, target):
        """Stage schedule[t] and let one tick pass, for every t, then run to quiescence; the last run's stats."""
        for dst, src, pay in self.schedule:
            if len(dst):
                target.tell(dst, pay, src)
            target.run(1)
        return target.run()


# ------------------------------------------------------------------ C2
def token_ring(n: int = 1_000_000, hops: int = 256, throughput: int = 5, tokens_per_actor: int = 1) -> Workload:
    """C2: every actor starts with `tokens_per_actor` tokens with hop budget H;
    RING behaviour: count++, forward payload-1 to (self+1) mod N while > 0.
    Delivered = tokens * N * (H + 1)."""
    dst = np.tile(np.arange(n, dtype=np.uint32), tokens_per_actor)
    pay = np.full(dst.size, hops, np.uint32)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("token_ring", n, 1, 1, throughput, 0, [(0, n, Kind.RING, None)], ring_stride=1,
                    tells=(dst, src, pay))


# ------------------------------------------------------------------ C3
def zipf_tables(n: int, s: float = 1.1, seed: int = SEED):
    """Zipf(s) over a seeded permutation of the actors, as u32 CDF thresholds:
    sample i = smallest i with u32(r >> 32) <= cdf[i]; actor = perm[i]."""
    ranks = np.arange(1, n + 1, dtype=np.float64)
    w = ranks ** (-s)
    cum = np.cumsum(w)
    cum /= cum[-1]
    cdf = np.floor(cum * 4294967296.0) - 1.0
    cdf = np.clip(cdf, 0, 4294967295.0).astype(np.uint64)
    cdf = np.maximum.accumulate(cdf)
    cdf[-1] = 0xFFFFFFFF
    key = splitmix64_np(np.arange(n, dtype=np.uint64) ^ np.uint64(seed))
    perm = np.argsort(key, kind="stable").astype(np.uint32)
    return cdf.astype(np.uint32), perm


def zipf_fanout(n: int = 10_000_000, k: int = 4, ttl: int = 3, root_every: int = 64, s: float = 1.1,
                throughput: int = 5, seed: int = SEED, capacity: int = 0) -> Workload:
    """C3: 1/root_every actors are roots holding one message with ttl; FANOUT
    behaviour: count++, sum += payload, if ttl > 0 emit k tells to Zipf targets."""
    cdf, perm = zipf_tables(n, s, seed)
    roots = np.arange(0, n, root_every, dtype=np.uint32)
    h = (splitmix64_np(roots.astype(np.uint64) ^ np.uint64(seed * 3)) & np.uint64(0x00FFFFFF)).astype(np.uint32)
    pay = (np.uint32(ttl) << np.uint32(24)) | h
    src = np.full(roots.size, NO_SENDER, np.uint32)
    return Workload("zipf_fanout", n, 2, k, throughput, capacity, [(0, n, Kind.FANOUT, None)],
                    fanout=(k, seed, cdf, perm), tells=(roots, src, pay.astype(np.uint32)))


# ------------------------------------------------------------------ C4
def crdt_ops(n: int, kind: int, ops_per_actor: int, seed: int = SEED):
    """Round-0 local updates, one row per actor: INCREMENT (GCounter), INCREMENT/DECREMENT
    (PNCounter), ADD/REMOVE of one of the 64 elements, 3:1 (ORSet)."""
    a = np.arange(n, dtype=np.uint64)
    out = np.zeros((n, ops_per_actor), np.uint32)
    for j in range(ops_per_actor):
        r = splitmix64_np((a << np.uint64(8)) ^ np.uint64(j) ^ np.uint64(seed * 11))
        lo = (r & np.uint64(0xFFFF)).astype(np.uint32)
        hi = ((r >> np.uint64(32)) & np.uint64(0xFF)).astype(np.uint32)
        if kind == Kind.GCOUNTER:
            op, arg = np.full(n, Op.INCREMENT, np.uint32), lo % 100 + 1
        elif kind == Kind.PNCOUNTER:
            op = np.where(hi % 3 == 0, Op.DECREMENT, Op.INCREMENT).astype(np.uint32)
            arg = lo % 100 + 1
        else:
            op = np.where(hi % 4 == 0, Op.REMOVE, Op.ADD).astype(np.uint32)
            arg = lo % 64
        out[:, j] = (op << np.uint32(24)) | arg
    return out


def crdt_gossip(n: int = 1_000_000, kind: int = Kind.GCOUNTER, rounds: int = 32, fanout: int = 2,
                ops_per_writer: int = 16, throughput: int = 5, seed: int = SEED, capacity: int = 0) -> Workload:
    """C4: Replicator-style replicas.  Actors 0..7 are the writers of node slots 0..7
    (one writer per UniqueAddress, as the CRDTs require) and first apply `ops_per_writer`
    local updates (host tells); then every actor runs `rounds` GossipTicks: each tick sends
    its full state to `fanout` random peers, which merge it
    (DD/Replicator.scala:2029-2064,2118-2133).  The population converges to the merge
    of the 8 writers' values."""
    nw = min(n, CRDT_NODES)
    ops = crdt_ops(nw, kind, ops_per_writer, seed).reshape(-1)
    odst = np.repeat(np.arange(nw, dtype=np.uint32), ops_per_writer)
    tdst = np.arange(n, dtype=np.uint32)
    tick = np.full(n, Op.make(Op.GOSSIP, rounds - 1), np.uint32)
    dst = np.concatenate([odst, tdst])
    pay = np.concatenate([ops, tick])
    src = np.full(dst.size, NO_SENDER, np.uint32)
    # a replica receives its tick + `fanout` gossips per superstep: buckets of 512 replicas keep
    # the ~3 x 512 messages in one 2048-message apply tile (the fast path)
    return Workload(f"crdt_gossip_{kind}", n, CRDT_WORDS[kind], fanout + 1, throughput, capacity,
                    [(0, n, kind, None)], gossip=(fanout, seed), tells=(dst, src, pay), bucket_actors=512)


def lwwmap_ops(nw: int, puts: int, removes: int, keys: int = 12, seed: int = SEED) -> np.ndarray:
    """Round-0 local updates of the `nw` writers of an LWWMap population, one row per writer: `puts` seeded puts
    with `removes` removes spread among them, all over the first `keys` keys, so that writers collide on keys."""
    per = puts + removes
    out = np.zeros((nw, per), np.uint32)
    a = np.arange(nw, dtype=np.uint64)
    rm_at = set((np.arange(removes) * per // max(removes, 1) + per // (2 * max(removes, 1))).tolist()) if removes else set()
    for j in range(per):
        r = splitmix64_np((a << np.uint64(8)) ^ np.uint64(j) ^ np.uint64(seed * 13))
        key = (r % np.uint64(keys)).astype(np.uint32)
        val = ((r >> np.uint64(20)) & np.uint64(0x3FFFF)).astype(np.uint32)
        if j in rm_at:
            out[:, j] = (np.uint32(Op.REMOVE) << np.uint32(24)) | key
        else:
            out[:, j] = (np.uint32(Op.PUT) << np.uint32(24)) | key | (val << np.uint32(6))
    return out


def crdt_lwwmap(n: int = 1_000_000, rounds: int = 32, fanout: int = 2, puts_per_writer: int = 16, removes: int = 4,
                throughput: int = 5, seed: int = SEED, capacity: int = 0, clock: str = "default", base: int = 0,
                bucket_actors: int = 512) -> Workload:
    """LWWMap replicas (LWWMap = ORMap of LWWRegister) in crdt_gossip's shape: replicas 0..7 are the writers, one
    per node slot, and first apply seeded puts and removes over a dozen keys (host tells), so that writers collide
    on keys; then every replica runs `rounds` GossipTicks.  The population converges to the merge of the writers'
    maps; the LWWRegister timestamps are logical time (`base` + superstep number) under `clock`."""
    nw = min(n, CRDT_NODES)
    per = puts_per_writer + removes
    ops = lwwmap_ops(nw, puts_per_writer, removes, seed=seed).reshape(-1)
    odst = np.repeat(np.arange(nw, dtype=np.uint32), per)
    tdst = np.arange(n, dtype=np.uint32)
    tick = np.full(n, Op.make(Op.GOSSIP, rounds - 1), np.uint32)
    dst = np.concatenate([odst, tdst])
    pay = np.concatenate([ops, tick])
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_lwwmap", n, CRDT_WORDS[Kind.LWWMAP], fanout + 1, throughput, capacity,
                    [(0, n, Kind.LWWMAP, None)], gossip=(fanout, seed), lwwmap=(clock, base), tells=(dst, src, pay),
                    bucket_actors=bucket_actors)


def pncountermap_ops(nw: int, incs: int, removes: int, keys: int = 12, seed: int = SEED) -> np.ndarray:
    """Round-0 local updates of the `nw` writers of a PNCounterMap population, one row per writer: `incs` seeded
    counts (about one in four a decrement, now and then by 0) with `removes` removes spread among them, all over the
    first `keys` keys, so that writers collide on keys."""
    per = incs + removes
    out = np.zeros((nw, per), np.uint32)
    a = np.arange(nw, dtype=np.uint64)
    rm_at = set((np.arange(removes) * per // max(removes, 1) + per // (2 * max(removes, 1))).tolist()) if removes else set()
    for j in range(per):
        r = splitmix64_np((a << np.uint64(8)) ^ np.uint64(j) ^ np.uint64(seed * 17))
        key = (r % np.uint64(keys)).astype(np.uint32)
        by = ((r >> np.uint64(20)) & np.uint64(0x3FFFF)).astype(np.uint32)
        by = np.where(((r >> np.uint64(40)) & np.uint64(15)) == 0, np.uint32(0), by)
        op = np.where(((r >> np.uint64(44)) & np.uint64(3)) == 0, np.uint32(Op.DECREMENT), np.uint32(Op.INCREMENT))
        if j in rm_at:
            out[:, j] = (np.uint32(Op.REMOVE) << np.uint32(24)) | key
        else:
            out[:, j] = (op << np.uint32(24)) | key | (by << np.uint32(6))
    return out


def crdt_pncountermap(n: int = 1_000_000, rounds: int = 32, fanout: int = 2, incs_per_writer: int = 16, removes: int = 4,
                      throughput: int = 5, seed: int = SEED, capacity: int = 0, bucket_actors: int = 512) -> Workload:
    """PNCounterMap replicas (PNCounterMap = ORMap of PNCounter) in crdt_lwwmap's shape: replicas 0..7 are the
    writers, one per node slot, and first apply seeded increments, decrements and removes over a dozen keys (host
    tells), so that writers collide on keys; then every replica runs `rounds` GossipTicks.  The population converges
    to the merge of the writers' maps.  A replica's snapshot row is up to 10 KB: pass `msg_capacity` to the engine
    explicitly (the default sizes the row heap for max(4n, 65536) messages)."""
    nw = min(n, CRDT_NODES)
    per = incs_per_writer + removes
    ops = pncountermap_ops(nw, incs_per_writer, removes, seed=seed).reshape(-1)
    odst = np.repeat(np.arange(nw, dtype=np.uint32), per)
    tdst = np.arange(n, dtype=np.uint32)
    tick = np.full(n, Op.make(Op.GOSSIP, rounds - 1), np.uint32)
    dst = np.concatenate([odst, tdst])
    pay = np.concatenate([ops, tick])
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_pncountermap", n, CRDT_WORDS[Kind.PNCOUNTERMAP], fanout + 1, throughput, capacity,
                    [(0, n, Kind.PNCOUNTERMAP, None)], gossip=(fanout, seed), tells=(dst, src, pay),
                    bucket_actors=bucket_actors)


def ormultimap_ops(nw: int, binds: int, removes: int, keys: int = 12, seed: int = SEED) -> np.ndarray:
    """Round-0 local updates of the `nw` writers of an ORMultiMap population, one row per writer -- a service
    registry: `binds` seeded binding ops (of 16, ten bind an instance to a service, three unbind one, one puts a
    whole set, two replace an instance) with `removes` removes of a whole service spread among them, all over the
    first `keys` services and the 8 instances, so that writers collide on keys and values."""
    per = binds + removes
    out = np.zeros((nw, per), np.uint32)
    a = np.arange(nw, dtype=np.uint64)
    rm_at = set((np.arange(removes) * per // max(removes, 1) + per // (2 * max(removes, 1))).tolist()) if removes else set()
    for j in range(per):
        r = splitmix64_np((a << np.uint64(8)) ^ np.uint64(j) ^ np.uint64(seed * 19))
        key = (r % np.uint64(keys)).astype(np.uint32)
        val = ((r >> np.uint64(20)) & np.uint64(7)).astype(np.uint32)
        new = ((r >> np.uint64(24)) & np.uint64(7)).astype(np.uint32)
        mask = ((r >> np.uint64(28)) & np.uint64(255)).astype(np.uint32)
        sel = ((r >> np.uint64(40)) & np.uint64(15)).astype(np.uint32)
        bind = (np.uint32(Op.ADD) << np.uint32(24)) | key | (val << np.uint32(6))
        unbind = (np.uint32(Op.REMOVE_BINDING) << np.uint32(24)) | key | (val << np.uint32(6))
        put = (np.uint32(Op.PUT) << np.uint32(24)) | key | (mask << np.uint32(6))
        repl = (np.uint32(Op.REPLACE_BINDING) << np.uint32(24)) | key | (val << np.uint32(6)) | (new << np.uint32(9))
        if j in rm_at:
            out[:, j] = (np.uint32(Op.REMOVE) << np.uint32(24)) | key
        else:
            out[:, j] = np.where(sel < 10, bind, np.where(sel < 13, unbind, np.where(sel < 14, put, repl)))
    return out


def crdt_ormultimap(n: int = 1_000_000, rounds: int = 32, fanout: int = 2, binds_per_writer: int = 16, removes: int = 4,
                    throughput: int = 5, seed: int = SEED, capacity: int = 0, bucket_actors: int = 512) -> Workload:
    """ORMultiMap replicas (ORMultiMap = ORMap of ORSet) as a service registry, in crdt_pncountermap's shape:
    replicas 0..7 are the writers, one per node slot, and first bind and unbind instances (8 values) to a dozen
    services (keys) with seeded host tells, so that writers collide on keys and values; then every replica runs
    `rounds` GossipTicks.  The population converges to the merge of the writers' maps.  A replica's snapshot row is
    up to 20 KB: pass `msg_capacity` to the engine explicitly (the default sizes the row heap for max(4n, 65536)
    messages)."""
    nw = min(n, CRDT_NODES)
    per = binds_per_writer + removes
    ops = ormultimap_ops(nw, binds_per_writer, removes, seed=seed).reshape(-1)
    odst = np.repeat(np.arange(nw, dtype=np.uint32), per)
    tdst = np.arange(n, dtype=np.uint32)
    tick = np.full(n, Op.make(Op.GOSSIP, rounds - 1), np.uint32)
    dst = np.concatenate([odst, tdst])
    pay = np.concatenate([ops, tick])
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_ormultimap", n, CRDT_WORDS[Kind.ORMULTIMAP], fanout + 1, throughput, capacity,
                    [(0, n, Kind.ORMULTIMAP, None)], gossip=(fanout, seed), tells=(dst, src, pay),
                    bucket_actors=bucket_actors)


def crdt_delta(n: int = 1_000_000, kind: int = Kind.ORSET, rounds: int = 32, write: bool = True,
               ops_per_replica: int = 0, gossip_rounds: int = 0, fanout: int = 1, max_delta_size: int = 50,
               throughput: int = 5, seed: int = SEED, capacity: int = 0, bucket_actors: int = 0) -> Workload:
    """C4 with delta-CRDT replication (Replicator delta-crdt.enabled, DD/Replicator.scala:1646-1695,
    1953-2027; DD/DeltaPropagationSelector.scala): keys of 8 replicas (id = 8 * key + node).  Each
    replica first applies `ops_per_replica` host updates, then runs `rounds` DeltaPropagationTicks
    (`write`: each tick also tells the replica one seeded Update, a writer client) and, if
    `gossip_rounds`, that many full-state GossipTicks to `fanout` random replicas of its key.
    bucket_actors 0: 2048 replicas per bucket (every bucket in the skew launch), measured after
    round 6's phase-B schedule against 512 / 1024: ORSet +8 %, GCounter +10 %."""
    if not bucket_actors:
        bucket_actors = 2048
    ids = np.arange(n, dtype=np.uint32)
    dsts, pays = [], []
    if ops_per_replica:
        dsts.append(np.repeat(ids, ops_per_replica))
        pays.append(crdt_ops(n, kind, ops_per_replica, seed).reshape(-1))
    if rounds:
        dsts.append(ids)
        pays.append(np.full(n, Op.make(Op.DELTA_TICK, (rounds - 1) | (DELTA_WRITE if write else 0)), np.uint32))
    if gossip_rounds:
        dsts.append(ids)
        pays.append(np.full(n, Op.make(Op.GOSSIP, gossip_rounds - 1), np.uint32))
    dst = np.concatenate(dsts)
    pay = np.concatenate(pays)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload(f"crdt_delta_{kind}", n, CRDT_DELTA_WORDS[kind], max(4, fanout + 1), throughput, capacity,
                    [(0, n, kind, None)], gossip=(fanout, seed), delta_crdt=max_delta_size, tells=(dst, src, pay),
                    bucket_actors=bucket_actors)


def crdt_lwwmap_delta(n: int = 1_000_000, rounds: int = 32, write: bool = True, ops_per_replica: int = 0,
                      gossip_rounds: int = 0, fanout: int = 1, max_delta_size: int = 50, throughput: int = 5,
                      seed: int = SEED, capacity: int = 0, clock: str = "default", base: int = 0,
                      bucket_actors: int = 512) -> Workload:
    """LWWMap replicas with delta replication (ORMap.DeltaOp; agx_set_lwwmap_delta) in crdt_delta's shape: keys of
    8 replicas (id = 8 * key + node).  Each replica first applies `ops_per_replica` host puts and removes
    (lwwmap_ops: about one remove in five, over a dozen keys), then runs `rounds` DeltaPropagationTicks (`write`:
    each tick also tells the replica one seeded put or remove, a writer client) and, if `gossip_rounds`, that many
    full-state GossipTicks to `fanout` random replicas of its key."""
    ids = np.arange(n, dtype=np.uint32)
    dsts, pays = [], []
    if ops_per_replica:
        removes = ops_per_replica // 5
        dsts.append(np.repeat(ids, ops_per_replica))
        pays.append(lwwmap_ops(n, ops_per_replica - removes, removes, seed=seed).reshape(-1))
    if rounds:
        dsts.append(ids)
        pays.append(np.full(n, Op.make(Op.DELTA_TICK, (rounds - 1) | (DELTA_WRITE if write else 0)), np.uint32))
    if gossip_rounds:
        dsts.append(ids)
        pays.append(np.full(n, Op.make(Op.GOSSIP, gossip_rounds - 1), np.uint32))
    dst = np.concatenate(dsts)
    pay = np.concatenate(pays)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_lwwmap_delta", n, LWWMAP_DELTA_WORDS, max(4, fanout + 1), throughput, capacity,
                    [(0, n, Kind.LWWMAP, None)], gossip=(fanout, seed), lwwmap=(clock, base), lwwmap_delta=max_delta_size,
                    tells=(dst, src, pay), bucket_actors=bucket_actors)


def crdt_delta_mixed(counts=(320, 320, 320), rounds: int = 8, throughput: int = 1, capacity: int = 0,
                     max_delta_size: int = 2, ops_per_replica: int = 3, gossip_rounds: int = 0, plain: int = 0,
                     big: bool = True, bucket_actors: int = 512, seed: int = SEED) -> Workload:
    """Delta-CRDT replication with all three data types in one engine: consecutive ranges of GCounter,
    ORSet and PNCounter replicas (`counts`), keys of 8 replicas by id as in crdt_delta -- so a key may
    straddle two ranges, and a group that reaches a replica of another type is Behaviors.unhandled --
    and `plain` COUNTER actors after them.  Every replica applies `ops_per_replica` host updates of
    its own type, then runs `rounds` writer DeltaPropagationTicks and, if `gossip_rounds`, that many
    full-state GossipTicks.  Counter rows and ORSet rows share one row heap at the ORSet pitch; with a
    low `throughput` the DeltaPropagations of every type wait in the mailboxes.
    `big`: the counters start at 2^40 | id in the replica's own increment slot (PNCounter: also
    3 * 2^41 | id in its own decrement slot), so both u32 halves of every delta value matter."""
    kinds = (Kind.GCOUNTER, Kind.ORSET, Kind.PNCOUNTER)
    W = CRDT_DELTA_WORDS[Kind.ORSET]
    n_crdt = int(sum(counts))
    n = n_crdt + plain
    ranges, dsts, pays = [], [], []
    first = 0
    for kd, count in zip(kinds, counts):
        ids = np.arange(first, first + count, dtype=np.uint32)
        init = None
        if big and kd != Kind.ORSET:
            init = np.zeros((count, W), np.uint64)
            rows = np.arange(count)
            init[rows, ids % CRDT_NODES] = (np.uint64(1) << np.uint64(40)) | ids.astype(np.uint64)
            if kd == Kind.PNCOUNTER:
                init[rows, CRDT_NODES + ids % CRDT_NODES] = (np.uint64(3) << np.uint64(41)) | ids.astype(np.uint64)
        ranges.append((first, count, kd, init))
        if ops_per_replica:
            dsts.append(np.repeat(ids, ops_per_replica))
            pays.append(crdt_ops(count, kd, ops_per_replica, seed + first).reshape(-1))
        first += count
    if plain:
        ranges.append((n_crdt, plain, Kind.COUNTER, None))
    ids = np.arange(n_crdt, dtype=np.uint32)
    if rounds:
        dsts.append(ids)
        pays.append(np.full(n_crdt, Op.make(Op.DELTA_TICK, (rounds - 1) | DELTA_WRITE), np.uint32))
    if gossip_rounds:
        dsts.append(ids)
        pays.append(np.full(n_crdt, Op.make(Op.GOSSIP, gossip_rounds - 1), np.uint32))
    dst = np.concatenate(dsts)
    pay = np.concatenate(pays)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_delta_mixed", n, W, 4, throughput, capacity, ranges, gossip=(1, seed),
                    delta_crdt=max_delta_size, tells=(dst, src, pay), bucket_actors=bucket_actors)


def crdt_mixed(n: int = 4096, rounds: int = 4, seed: int = 3, throughput: int = 3, capacity: int = 0) -> Workload:
    """GCounter / PNCounter / ORSet replicas beside COUNTER and EVEN actors: gossips that
    land on a non-CRDT actor (or an ORSet op on a counter) are Behaviors.unhandled."""
    kinds = [Kind.GCOUNTER, Kind.PNCOUNTER, Kind.ORSET, Kind.COUNTER, Kind.EVEN]
    per = n // len(kinds)
    ranges, dsts, pays = [], [], []
    rng = np.random.default_rng(seed)
    for i, kd in enumerate(kinds):
        first = i * per
        count = per if i < len(kinds) - 1 else n - first
        ranges.append((first, count, kd, None))
        ids = np.arange(first, first + count, dtype=np.uint32)
        if kd in CRDT_WORDS:
            ops = crdt_ops(count, kd, 3, seed + i)
            tick = np.full((count, 1), Op.make(Op.GOSSIP, rounds - 1), np.uint32)
            dsts.append(np.repeat(ids, 4))
            pays.append(np.concatenate([ops, tick], axis=1).reshape(-1))
    m = n
    dsts.append(rng.integers(0, n, m).astype(np.uint32))  # random control ops everywhere
    pays.append(((rng.integers(1, 8, m).astype(np.uint32) << 24) | rng.integers(0, 70, m).astype(np.uint32)))
    dst = np.concatenate(dsts)
    pay = np.concatenate(pays)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("crdt_mixed", n, CRDT_WORDS[Kind.ORSET], 3, throughput, capacity, ranges, gossip=(2, seed),
                    tells=(dst, src, pay))


# ------------------------------------------------------------------ C5
RMAT_ABC = (0.57, 0.19, 0.19)


def power_law_degrees(n: int, alpha: float = 2.1, dmax: int = 1024, seed: int = SEED) -> np.ndarray:
    """CSR row pointer (u64, n+1) of out-degrees ~ d^-alpha on [1, dmax], one integer
    draw per actor against host-built u32-scaled thresholds."""
    d = np.arange(1, dmax + 1, dtype=np.float64)
    p = d ** (-alpha)
    cdf = np.cumsum(p) / p.sum()
    thr = np.floor(cdf * 4294967296.0).astype(np.uint64)
    thr[-1] = 1 << 32
    row = np.zeros(n + 1, np.uint64)
    for lo in range(0, n, 1 << 24):  # chunked: bounded temporaries at 10^8 actors
        hi = min(n, lo + (1 << 24))
        r = splitmix64_np(np.arange(lo, hi, dtype=np.uint64) ^ np.uint64(seed * 7)) >> np.uint64(32)
        deg = np.minimum(np.searchsorted(thr, r, side="right") + 1, dmax).astype(np.uint64)
        row[lo + 1:hi + 1] = deg
    np.cumsum(row, out=row)
    return row


def rmat_params(n: int, a: float = RMAT_ABC[0], b: float = RMAT_ABC[1], c: float = RMAT_ABC[2],
                seed: int = SEED) -> tuple:
    """(bits, ta, tb, tc, seed) of the R-MAT destination draw (agx_set_graph_rmat)."""
    bits = max(1, int(np.ceil(np.log2(max(n, 2)))))
    return bits, int(a * 65536), int((a + b) * 65536), int((a + b + c) * 65536), seed


def rmat_cols(m: int, n: int, bits: int, ta: int, tb: int, tc: int, seed: int) -> np.ndarray:
    """Destination of every edge id in [0, m): `bits` quadrant draws q = splitmix64(e*64 + bit +
    seed) & 0xFFFF, destination bit = (ta <= q < tb) | (q >= tc), reduced mod n."""
    col = np.zeros(m, np.uint64)
    eid = np.arange(m, dtype=np.uint64)
    for bit in range(bits):
        rr = splitmix64_np(eid * np.uint64(64) + np.uint64(bit) + np.uint64(seed)) & np.uint64(0xFFFF)
        dst_bit = ((rr >= np.uint64(ta)) & (rr < np.uint64(tb))) | (rr >= np.uint64(tc))
        col |= dst_bit.astype(np.uint64) << np.uint64(bits - 1 - bit)
    col %= np.uint64(n)
    return col.astype(np.uint32)


def power_law_graph(n: int, alpha: float = 2.1, dmax: int = 1024, a: float = RMAT_ABC[0], b: float = RMAT_ABC[1],
                    c: float = RMAT_ABC[2], seed: int = SEED):
    """Out-degrees ~ d^-alpha on [1, dmax]; endpoints by R-MAT bit sampling.
    Integer RNG throughout (float only to build the host-side degree table)."""
    row = power_law_degrees(n, alpha, dmax, seed)
    return row, rmat_cols(int(row[-1]), n, *rmat_params(n, a, b, c, seed))


def power_law_forward(n: int = 100_000_000, ttl: int = 16, capacity: int = 64, throughput: int = 5,
                      msgs_per_actor_den: int = 1, seed: int = SEED, device_graph: bool = False) -> Workload:
    """C5: FORWARD_RR over a power-law graph with BoundedMailbox(capacity).
    device_graph: the R-MAT destinations are generated by the engine (agx_set_graph_rmat);
    targets without that entry point (the CPU oracle) get them from rmat_cols."""
    row = power_law_degrees(n, seed=seed)
    graph = ("rmat", row, rmat_params(n, seed=seed)) if device_graph else (row, rmat_cols(
        int(row[-1]), n, *rmat_params(n, seed=seed)))
    dst = np.arange(0, n, msgs_per_actor_den, dtype=np.uint32)
    pay = np.full(dst.size, ttl, np.uint32)
    src = np.full(dst.size, NO_SENDER, np.uint32)
    return Workload("power_law_forward", n, 2, 1, throughput, capacity, [(0, n, Kind.FORWARD_RR, None)],
                    graph=graph, tells=(dst, src, pay))


# ------------------------------------------------------------------ C1
def ping_pong(pairs: int = 1000, messages_per_pair: int = 2_000_000, throughput: int = 50,
              in_flight: int | None = None) -> Workload:
    """C1: BenchmarkActors.PingPong pairs (akka-bench-jmh/.../BenchmarkActors.scala:20-32,96-117):
    left = messagesPerPair/2 per actor, inFlight = 2*throughput initial tells
    `ping.tell(Message, pong)` per pair."""
    if in_flight is None:
        in_flight = 2 * throughput
    n = 2 * pairs
    init = np.zeros((n, 2), np.uint64)
    init[:, 0] = messages_per_pair // 2
    ping = np.arange(0, n, 2, dtype=np.uint32)
    dst = np.repeat(ping, in_flight)
    src = dst + np.uint32(1)
    pay = np.zeros(dst.size, np.uint32)
    # in_flight tells per pair: ~in_flight/2 queued per actor -> buckets of 2048/in_flight actors fit one tile
    ba = max(32, min(2048, 1 << max(0, (2048 // max(in_flight, 1)).bit_length() - 1)))
    return Workload("ping_pong", n, 2, 1, throughput, 0, [(0, n, Kind.PINGPONG, init)], tells=(dst, src, pay),
                    bucket_actors=ba)


# ------------------------------------------------------------------ small mixed workload for parity tests
def mixed(n: int = 4096, seed: int = 1, throughput: int = 3, capacity: int = 0, tells_per_actor: int = 3) -> Workload:
    """Every behaviour kind side by side (ranges), random tells between them."""
    rng = np.random.default_rng(seed)
    kinds = [Kind.COUNTER, Kind.RING, Kind.FANOUT, Kind.FORWARD_RR, Kind.STOP_AFTER, Kind.PINGPONG, Kind.EVEN,
             Kind.NONE]
    per = n // len(kinds)
    ranges = []
    for i, kd in enumerate(kinds):
        first = i * per
        count = per if i < len(kinds) - 1 else n - first
        init = None
        if kd == Kind.STOP_AFTER:
            init = np.zeros((count, 2), np.uint64)
            init[:, 1] = rng.integers(1, 6, count)
        elif kd == Kind.PINGPONG:
            init = np.zeros((count, 2), np.uint64)
            init[:, 0] = rng.integers(0, 5, count)
        ranges.append((first, count, kd, init))
    cdf, perm = zipf_tables(n, 1.1, seed)
    row, col = power_law_graph(n, seed=seed)
    m = n * tells_per_actor
    dst = rng.integers(0, n + 8, m).astype(np.uint32)  # a few unknown refs -> dead letters
    src = rng.integers(0, n, m).astype(np.uint32)
    src[rng.random(m) < 0.1] = NO_SENDER
    pay = rng.integers(0, 12, m).astype(np.uint32)
    # fan-out payloads carry ttl in the top 8 bits
    fan_first, fan_count = ranges[2][0], ranges[2][1]
    is_fan = (dst >= fan_first) & (dst < fan_first + fan_count)
    pay[is_fan] = (rng.integers(0, 3, int(is_fan.sum())).astype(np.uint32) << 24) | rng.integers(
        0, 1 << 24, int(is_fan.sum())).astype(np.uint32)
    return Workload("mixed", n, 2, 2, throughput, capacity, ranges, ring_stride=7, fanout=(2, seed, cdf, perm),
                    graph=(row, col), tells=(dst, src, pay))


def one_per_actor(n: int = 4096, seed: int = 1, throughput: int = 3, capacity: int = 0, compiled_kinds: bool = False,
                  n_host: int = 16) -> Workload:
    """mixed()'s behaviour kinds (or the compiled library with `compiled_kinds`) with exactly one
    staged tell per actor (a permutation of the population): buckets whose inbox holds at most one
    message per actor (the dense path, agx_kernels.h dense_finish) beside buckets where forwards
    collide; stops, dead letters to stopped actors, unknown refs and replies to host-side actors
    (PINGPONG -> outbox) included."""
    rng = np.random.default_rng(seed)
    w = compiled(n, seed=seed, throughput=throughput, capacity=capacity, builtin=True) if compiled_kinds else \
        mixed(n, seed=seed, throughput=throughput, capacity=capacity)
    dst = rng.permutation(n).astype(np.uint32)
    src = rng.integers(0, n, n).astype(np.uint32)
    src[rng.random(n) < 0.1] = NO_SENDER
    if n_host:
        hs = rng.random(n) < 0.05
        src[hs] = rng.integers(n, n + n_host, int(hs.sum())).astype(np.uint32)
        w.outbound = (n, n_host)
    pay = rng.integers(0, 12, n).astype(np.uint32)
    if not compiled_kinds:  # fan-out payloads carry ttl in the top 8 bits
        fan_first, fan_count = w.ranges[2][0], w.ranges[2][1]
        is_fan = (dst >= fan_first) & (dst < fan_first + fan_count)
        pay[is_fan] = (rng.integers(0, 3, int(is_fan.sum())).astype(np.uint32) << 24) | rng.integers(
            0, 1 << 24, int(is_fan.sum())).astype(np.uint32)
    w.name = "one_per_actor"
    w.tells = (dst, src, pay)
    return w


def compiled(n: int = 4096, seed: int = 1, throughput: int = 3, capacity: int = 0, tells_per_actor: int = 3,
             builtin: bool = False) -> Workload:
    """Typed behaviours lowered by akka_amd.typed (compiled behaviour tables): the DSL versions of
    counter / ring / stop-after / ping-pong and a pair of behaviours that become each other, side
    by side (and beside the built-in kinds with `builtin`), random tells between them."""
    from . import typed
    rng = np.random.default_rng(seed)
    lib = typed.library(ring_stride=7)
    sw = typed.switch()
    tables = typed.compile_behaviors([lib["counter"], lib["ring"], lib["stop_after"], lib["ping_pong"], sw])
    kinds = [tables.kind_of(lib[k]) for k in ("counter", "ring", "stop_after", "ping_pong")] + [tables.kind_of(sw)]
    if builtin:
        kinds += [Kind.COUNTER, Kind.RING, Kind.PINGPONG, Kind.STOP_AFTER]
    per = n // len(kinds)
    ranges = []
    for i, kd in enumerate(kinds):
        first = i * per
        count = per if i < len(kinds) - 1 else n - first
        init = None
        if kd in (tables.kind_of(lib["stop_after"]), Kind.STOP_AFTER):
            init = np.zeros((count, 2), np.uint64)
            init[:, 1] = rng.integers(1, 6, count)
        elif kd in (tables.kind_of(lib["ping_pong"]), Kind.PINGPONG):
            init = np.zeros((count, 2), np.uint64)
            init[:, 0] = rng.integers(0, 5, count)
        ranges.append((first, count, kd, init))
    m = n * tells_per_actor
    dst = rng.integers(0, n + 8, m).astype(np.uint32)  # a few unknown refs -> dead letters
    src = rng.integers(0, n, m).astype(np.uint32)
    src[rng.random(m) < 0.1] = NO_SENDER
    pay = rng.integers(0, 12, m).astype(np.uint32)
    sw_first, sw_count = ranges[4][0], ranges[4][1]
    is_sw = (dst >= sw_first) & (dst < sw_first + sw_count)
    k = int(is_sw.sum())
    pay[is_sw] = (rng.integers(1, 4, k).astype(np.uint32) << 24) | rng.integers(0, 6, k).astype(np.uint32)
    return Workload("compiled", n, 2, 1, throughput, capacity, ranges, ring_stride=7, tells=(dst, src, pay),
                    behaviors=tables)


def compiled_ring(n: int = 1_000_000, hops: int = 256, throughput: int = 5) -> Workload:
    """C2's token ring with the ring behaviour written in the typed DSL (akka_amd.typed.library)."""
    from . import typed
    ring = typed.library(ring_stride=1)["ring"]
    tables = typed.compile_behaviors([ring])
    w = token_ring(n, hops, throughput)
    w.name, w.ranges, w.behaviors = "compiled_ring", [(0, n, tables.kind_of(ring), None)], tables
    return w


# ------------------------------------------------------------------ per-actor mailboxes + the reply path
def mailbox_mix(n: int = 4096, seed: int = 7, throughput: int = 3, capacity: int = 0, n_host: int = 32,
                tells_per_actor: int = 3, classes: dict | None = None) -> Workload:
    """mixed() with several mailbox types in one dispatcher (Mailboxes.lookupConfigurator per actor,
    Mailboxes.scala:204-260): quarters of the population bound to bounded-capacity:2, an unbounded
    type, bounded-capacity:16 and the dispatcher default (`capacity`) -- or `classes` {class: capacity}
    for classes 1..3; plus `n_host` host-side actors
    (ids n..n+n_host-1, e.g. JVM TestProbes) that tell GPU actors -- PINGPONG actors answer them
    through the outbox (sender() ! reply, ActorCell.scala:583-587)."""
    w = mixed(n, seed=seed, throughput=throughput, capacity=capacity, tells_per_actor=tells_per_actor)
    q = n // 4
    w.name = "mailbox_mix"
    w.mailbox_classes = dict(classes) if classes else {1: 2, 2: 0, 3: 16}
    w.mailboxes = [(0, q, 1), (q, q, 2), (2 * q, q, 3)]
    if n_host:
        w.outbound = (n, n_host)
        rng = np.random.default_rng(seed + 101)
        m = max(1, n // 4)
        dst, src, pay = w.tells
        hs = rng.integers(n, n + n_host, m).astype(np.uint32)
        hd = rng.integers(0, n, m).astype(np.uint32)
        hp = rng.integers(0, 12, m).astype(np.uint32)
        # host senders to every kind; the PINGPONG range answers them
        w.tells = (np.concatenate([dst, hd]), np.concatenate([src, hs]), np.concatenate([pay, hp]))
    return w


# ------------------------------------------------------------------ priority and control-aware mailboxes
PRIORITY_MIX_STOP_TAG = 9


def priority_mix(n: int = 2048, seed: int = 1, throughput: int = 3, n_host: int = 8, tells_per_actor: float = 0.7,
                 tables: bool = True) -> Workload:
    """Four mailbox types in one dispatcher, two of them prioritised (agx_set_mailbox_priority;
    Unbounded/BoundedStablePriorityMailbox, Mailbox.scala:726-816): quarters of the population on
    class 1 (prioritised, unbounded), class 2 (prioritised, capacity 4), class 3 (FIFO, capacity 2)
    and class 0 (FIFO, unbounded).  The actors are compiled relays (typed.forwarder, hops 1 and 5)
    that pass tagged messages on with one hop less, echo the messages of host-side senders through
    the outbox and stop on tag PRIORITY_MIX_STOP_TAG.  Destinations are skewed inside groups of 64
    actors (offset 64 u^3), so many actors hold 2-40 messages while a bucket's load stays near
    `tells_per_actor` per actor.  `tables=False`: the same population with every class FIFO."""
    from . import typed
    rng = np.random.default_rng(seed)
    fa, fb = typed.forwarder(n, 1, PRIORITY_MIX_STOP_TAG), typed.forwarder(n, 5, PRIORITY_MIX_STOP_TAG)
    tb = typed.compile_behaviors([fa, fb], max_emit=1)
    h = n // 2
    ranges = [(0, h, tb.kind_of(fa), None), (h, n - h, tb.kind_of(fb), None)]
    m = max(1, int(n * tells_per_actor))
    group = (rng.integers(0, max(1, n // 64), m) * 64).astype(np.int64)
    dst = np.minimum(group + (64 * rng.random(m) ** 3).astype(np.int64), n - 1).astype(np.uint32)
    src = rng.integers(0, n, m).astype(np.uint32)
    if n_host:
        hs = rng.random(m) < 0.15
        src[hs] = rng.integers(n, n + n_host, int(hs.sum())).astype(np.uint32)
    tag = rng.integers(1, 8, m).astype(np.uint32)
    tag[rng.random(m) < 0.03] = PRIORITY_MIX_STOP_TAG
    pay = (tag << np.uint32(24)) | rng.integers(0, 6, m).astype(np.uint32)
    prio = bytes([3, 0, 2, 1, 2, 0, 3, 1][t % 8] for t in range(256))  # (the stop tag overtakes: priority 0)
    q = n // 4
    return Workload("priority_mix", n, 2, 1, throughput, 0, ranges, behaviors=tb, tells=(dst, src, pay),
                    mailbox_classes={1: 0, 2: 4, 3: 2}, mailboxes=[(0, q, 1), (q, q, 2), (2 * q, q, 3)],
                    outbound=(n, n_host) if n_host else None,
                    mailbox_priorities={1: prio, 2: prio} if tables else {})


# ------------------------------------------------------------------ deque-based mailboxes: the stash
GATE_OPEN, GATE_CLOSE, GATE_DATA, GATE_STOP = 1, 2, 3, 4
STASH_GATE_HOP = 67


def gate(n_actors: int, capacity: int, hop: int = STASH_GATE_HOP):
    """(closed, open): a gate as two behaviours around one StashBuffer (Behaviors.withStash; "buffer until
    initialised, then replay", the first pattern of the reference's stash documentation).  Closed, it
    stashes every data message; Open releases them into the open gate (unstash_all) and Close shuts it
    again.  Open, a data message of a host-side sender is echoed to it, any other one with a hop count
    above 0 goes on to the actor `hop` ids further with one hop less; a second Open releases what was
    stashed meanwhile.  Stop stops the gate.  State: messages seen (a stashed one twice), the last
    payload handled while open."""
    from . import typed
    st = typed.State("count", "last")
    tag = lambda t: (lambda m: m.tag == t)

    def build(buf):
        closed, opened = typed.Behavior("closed", st), typed.Behavior("open", st)
        seen = lambda m, s: [s.count.inc(), s.last.set(m.payload)]
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [s.count.inc(), buf.unstash_all(opened)], test=tag(GATE_OPEN))
         .on_any_message(lambda m, s: [typed.Behaviors.same], test=tag(GATE_CLOSE))
         .on_any_message(lambda m, s: [s.count.inc(), typed.Behaviors.stopped], test=tag(GATE_STOP))
         .on_any_message(lambda m, s: [s.count.inc(), buf.stash(), typed.Behaviors.same])
         .build(into=closed))
        (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [closed], test=tag(GATE_CLOSE))
         .on_any_message(lambda m, s: [s.count.inc(), buf.unstash_all(typed.Behaviors.same)], test=tag(GATE_OPEN))
         .on_any_message(lambda m, s: [s.count.inc(), typed.Behaviors.stopped], test=tag(GATE_STOP))
         .on_any_message(lambda m, s: seen(m, s) + [m.sender.tell(m.payload), typed.Behaviors.same],
                         test=lambda m: m.sender.dst >= n_actors)
         .on_any_message(lambda m, s: seen(m, s) + [typed.self_ref(hop).tell(m.payload - 1), typed.Behaviors.same],
                         test=lambda m: m.arg > 0)
         .on_any_message(lambda m, s: seen(m, s) + [typed.Behaviors.same])
         .build(into=opened))
        return closed

    closed = typed.Behaviors.with_stash(capacity, build)
    return closed, closed.cases[0].result.target


def stash_gate(n: int = 2048, seed: int = 1, throughput: int = 3, n_host: int = 8, tells_per_actor: float = 0.9,
               all_open: bool = False) -> Workload:
    """A population of gates (gate() above) on four mailbox types: halves of the population start closed
    and open; quarters are bound to class 1 (unbounded deque-based, stash-capacity 12), class 2
    (bounded-capacity 4, deque-based, stash-capacity 3), class 3 (bounded-capacity 8, no stash: a gate
    of it that stashes fails at once) and class 0 (the dispatcher default, stash-capacity 2).  Host
    tells: data messages with hop counts (some from host-side senders, echoed through the outbox: the
    order observable), Open, Close and a few Stop, skewed inside groups of 64 actors as priority_mix.
    `all_open`: every gate starts open and no Close is sent -- the same traffic without a stash in use."""
    from . import typed
    rng = np.random.default_rng(seed)
    closed, opened = gate(n, 12)
    tb = typed.compile_behaviors([closed, opened], max_emit=1)
    h = n // 2
    ranges = [(0, h, tb.kind_of(opened if all_open else closed), None), (h, n - h, tb.kind_of(opened), None)]
    m = max(1, int(n * tells_per_actor))
    group = (rng.integers(0, max(1, n // 64), m) * 64).astype(np.int64)
    dst = np.minimum(group + (64 * rng.random(m) ** 3).astype(np.int64), n - 1).astype(np.uint32)
    src = rng.integers(0, n, m).astype(np.uint32)
    if n_host:
        hs = rng.random(m) < 0.3
        src[hs] = rng.integers(n, n + n_host, int(hs.sum())).astype(np.uint32)
    u = rng.random(m)
    tag = np.full(m, GATE_DATA, np.uint32)
    tag[u < 0.24] = GATE_OPEN
    tag[u < 0.10] = GATE_DATA if all_open else GATE_CLOSE
    tag[u < 0.02] = GATE_STOP
    pay = (tag << np.uint32(24)) | rng.integers(0, 7, m).astype(np.uint32)
    late = np.argsort(tag == GATE_OPEN, kind="stable")  # the Opens are told last: a closed gate has buffered by then
    dst, src, pay = dst[late], src[late], pay[late]
    q = n // 4
    return Workload("stash_gate", n, 2, 1, throughput, 0, ranges, behaviors=tb, tells=(dst, src, pay),
                    mailbox_classes={1: 0, 2: 4, 3: 8}, mailboxes=[(0, q, 1), (q, q, 2), (2 * q, q, 3)],
                    outbound=(n, n_host) if n_host else None, bucket_actors=128,
                    stash={0: 2, 1: 12, 2: 3})


# ------------------------------------------------------------------ timers: a population of heartbeats
HB_TICK, HB_PING, HB_CANCEL, HB_REPLACE, HB_ECHO, HB_STOP = 1, 2, 3, 4, 5, 6


def heartbeater():
    """A failure-detector style actor (Behaviors.withTimers): every Tick of its periodic timer "hb" it counts
    the beat and pings its neighbour, which counts the ping.  Cancel cancels the timer, Replace(d) restarts it
    with period d + 1 (a new generation: a Tick already in the mailbox is discarded), Echo answers the sender
    with the beat count, Stop stops the actor (its timer with it)."""
    from . import typed
    st = typed.State("beats", "pings")
    B = typed.Behaviors
    tick = typed.MessageType("Tick", HB_TICK)
    is_ = lambda t: (lambda m: m.tag == t)

    def build(timers):
        return (typed.ReceiveBuilder.create(st)
                .on_any_message(lambda m, s: [s.beats.inc(), typed.self_ref(1).tell(s.beats, tag=HB_PING), B.same],
                                test=is_(HB_TICK))
                .on_any_message(lambda m, s: [s.pings.inc(), B.same], test=is_(HB_PING))
                .on_any_message(lambda m, s: [timers.cancel("hb"), B.same], test=is_(HB_CANCEL))
                .on_any_message(lambda m, s: [timers.start_timer_with_fixed_delay("hb", tick(m.arg), m.arg + 1), B.same],
                                test=is_(HB_REPLACE))
                .on_any_message(lambda m, s: [m.sender.tell(s.beats, tag=HB_ECHO), B.same], test=is_(HB_ECHO))
                .on_any_message(lambda m, s: [B.stopped], test=is_(HB_STOP))
                .on_any_message(lambda m, s: [B.unhandled])
                .build("heartbeater"))
    return B.with_timers(build)


def heartbeat(n: int = 1 << 20, period: int = 16, seed: int = 1, throughput: int = 3, n_host: int = 8,
              host_fraction: float = 0.05, bucket_actors: int = 0) -> Workload:
    """Every actor starts a periodic timer of `period` ticks with a staggered phase (the first fire after
    1..period ticks); each Tick it counts the beat and pings its neighbour.  A fraction of the actors get a host
    message at the start: Cancel, Replace (another period), Stop, or Echo from a host-side sender (answered
    through the outbox: the order observable).  A periodic timer never lets the engine go quiescent: run it
    with a budget.  An engine with timers keeps a bucket's inbox within one 2048-message tile (agx_set_timers),
    and every tick brings about 2 / period messages per actor (the Tick and the neighbour's ping), so choose
    `bucket_actors` below 1024 x period: at period 1 the default 2048-actor bucket is refused with
    AGX_ECAPACITY, 512-actor buckets run."""
    from . import typed
    rng = np.random.default_rng(seed)
    b = heartbeater()
    tb = typed.compile_behaviors([b], max_emit=1)
    delays = (1 + rng.integers(0, max(period, 1), n)).astype(np.uint32)
    m = int(n * host_fraction)
    tells = None
    if m:
        dst = rng.integers(0, n, m).astype(np.uint32)
        u = rng.random(m)
        tag = np.full(m, HB_ECHO, np.uint32)
        tag[u < 0.6] = HB_REPLACE
        tag[u < 0.35] = HB_CANCEL
        tag[u < 0.1] = HB_STOP
        src = rng.integers(0, n, m).astype(np.uint32)
        if n_host:
            e = tag == HB_ECHO
            src[e] = rng.integers(n, n + n_host, int(e.sum())).astype(np.uint32)
        pay = (tag << np.uint32(24)) | rng.integers(0, 2 * max(period, 1), m).astype(np.uint32)
        tells = (dst, src, pay)
    return Workload("heartbeat", n, 2, 1, throughput, 0, [(0, n, tb.kind_of(b), None)], behaviors=tb, tells=tells,
                    outbound=(n, n_host) if n_host else None, bucket_actors=bucket_actors,
                    timers={"n_keys": tb.timer_keys,
                            "starts": [(0, n, 0, True, period, delays, (HB_TICK << 24))]})


# ------------------------------------------------------------------ receive timeouts: entities that passivate
PE_JOB, PE_IDLE, PE_PASSIVATE, PE_STOP = 1, 2, 3, 4


def passivating_entity():
    """A sharded entity and its shard (ShardRegion.Passivate's handshake, ShardRegion.scala:188-199): the entity
    counts its jobs; idle for its receive timeout it receives Idle and tells its shard (state word 1) Passivate; the
    shard counts it and answers the sender with StopEntity, on which the entity stops.  One tell per case."""
    from . import typed
    B = typed.Behaviors
    job, idle, passivate, stop = (typed.MessageType(n, t) for n, t in
                                  (("Job", PE_JOB), ("Idle", PE_IDLE), ("Passivate", PE_PASSIVATE), ("StopEntity", PE_STOP)))
    es = typed.State("jobs", "shard")
    entity = (typed.ReceiveBuilder.create(es)
              .on_message(job, lambda m, s: [s.jobs.inc(), B.same])
              .on_message(idle, lambda m, s: [s.shard.ref.tell(passivate()), B.same])
              .on_message(stop, lambda m, s: [B.stopped])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("entity"))
    ss = typed.State("passivated", "unused")
    shard = (typed.ReceiveBuilder.create(ss)
             .on_message(passivate, lambda m, s: [s.passivated.inc(), m.sender.tell(stop()), B.same])
             .on_any_message(lambda m, s: [B.unhandled])
             .build("shard"))
    return entity, shard


def passivating_entities(n: int = 1 << 20, n_shards: int = 4096, idle: int = 8, seed: int = 1, throughput: int = 16,
                         bucket_actors: int = 256, spread: int | None = None, set_timeouts: bool = True) -> Workload:
    """Entities (ids 0..n-1, shard n + i mod n_shards) set a receive timeout of `idle` ticks (the setup block) and
    count the jobs the host sends them by a decaying schedule (Workload.schedule, run_schedule): entity i gets one
    job per tick up to a last tick drawn from a geometric distribution cut at `spread` ticks (default
    min(256, max(8, n / 8)); about 4 / spread of the entities still busy fall silent per tick).  `idle` ticks
    after its last job an entity receives Idle and passivates: Passivate to its shard, StopEntity back, stop.  The
    run goes quiescent once every entity has passivated; the engine needs timer_keys 1 though no timer is used.
    An engine with timers keeps a bucket's inbox within one 2048-message tile, and the shards of one bucket take
    every Passivate of their entities in the tick it is sent: keep n * 4 / spread below 2048 * n_shards /
    bucket_actors (the defaults: 16384 a tick on 16 buckets of shards).  A shard that gets more Passivates in a tick
    than `throughput` answers the rest later; an entity still alive `idle` ticks on asks again, as the reference's
    would.  `set_timeouts=False`: the same traffic on
    the same engine with no timeout ever set (no entity passivates) -- what the per-message reset costs."""
    from . import typed
    rng = np.random.default_rng(seed)
    entity, shard = passivating_entity()
    tb = typed.compile_behaviors([entity, shard], max_emit=1)
    spread = min(256, max(8, n // 8)) if spread is None else spread
    decay = 1.0 - min(4.0 / spread, 0.5)
    last = np.minimum(np.floor(np.log(1.0 - rng.random(n)) / np.log(decay)), spread - 1).astype(np.int64)
    ids = np.arange(n, dtype=np.uint32)
    schedule = []
    for t in range(spread):
        dst = ids[last >= t]
        schedule.append((dst, np.full(dst.size, NO_SENDER, np.uint32), np.full(dst.size, PE_JOB << 24, np.uint32)))
    init = np.zeros((n, 2), np.uint64)
    init[:, 1] = n + ids % n_shards
    rt = {"transparent": (), "starts": [(0, n, idle, PE_IDLE << 24)] if set_timeouts else []}
    return Workload("passivating_entities", n + n_shards, 2, 1, throughput, 0,
                    [(0, n, tb.kind_of(entity), init), (n, n_shards, tb.kind_of(shard), None)], behaviors=tb,
                    bucket_actors=bucket_actors, schedule=schedule,
                    timers={"n_keys": max(tb.timer_keys, 1), "receive_timeout": rt})


# ------------------------------------------------------------------ sharded entities: start on demand, Passivate, restart
SE_JOB, SE_IDLE, SE_BYE, SE_PASSIVATE, SE_STOP = 1, 2, 3, 4, 5


def sharded_entity():
    """An entity of a shard (akka-cluster-sharding Shard.scala:388-516) and a plain actor beside it: the entity counts
    the jobs of its incarnation (state word 0; word 1 is its id); Idle -- its receive timeout -- and a host's
    Passivate make it context.passivate(); Bye is its stop message; Stop is a crash-like plain stop."""
    from . import typed
    B = typed.Behaviors
    job, idle, bye, passivate, stop = (typed.MessageType(n, t) for n, t in
                                       (("Job", SE_JOB), ("Idle", SE_IDLE), ("Bye", SE_BYE), ("Passivate", SE_PASSIVATE),
                                        ("Stop", SE_STOP)))
    es = typed.State("jobs", "id")
    entity = (typed.ReceiveBuilder.create(es)
              .on_message(job, lambda m, s: [s.jobs.inc(), B.same])
              .on_message(idle, lambda m, s: [typed.context.passivate(), B.same])
              .on_message(passivate, lambda m, s: [typed.context.passivate(), B.same])
              .on_message(bye, lambda m, s: [B.stopped])
              .on_message(stop, lambda m, s: [B.stopped])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("sharded_entity"))
    ps = typed.State("jobs", "unused")
    plain = (typed.ReceiveBuilder.create(ps)
             .on_message(job, lambda m, s: [s.jobs.inc(), B.same])
             .on_any_message(lambda m, s: [B.unhandled])
             .build("plain"))
    return entity, plain, bye, idle


def _sharded(name, n, n_plain, idle, throughput, bucket_actors, schedule, capacity=0) -> Workload:
    from . import typed
    entity, plain, bye, idle_msg = sharded_entity()
    ent = typed.Entity(typed.EntityTypeKey("job-counter"), entity, n_plain, n, word1=typed.Entity.ID).with_stop_message(bye())
    if idle:
        ent = ent.with_receive_timeout(idle, idle_msg())
    tb = typed.compile_behaviors([plain], max_emit=1, entities=[ent])
    rt = {"transparent": (), "starts": [], "sharding": tb.entity_types}
    return Workload(name, n_plain + n, 2, 1, throughput, capacity, [(0, n_plain, tb.kind_of(plain), None)] if n_plain else [],
                    behaviors=tb, bucket_actors=bucket_actors, schedule=schedule,
                    timers={"n_keys": max(tb.timer_keys, 1), "receive_timeout": rt})


def sharded_entities(n: int = 1 << 20, idle: int = 4, ticks: int = 64, seed: int = 1, throughput: int = 16,
                     bucket_actors: int = 256, n_plain: int = 8, p_passivate: float = 0.01, p_stop: float = 0.005) -> Workload:
    """`n` entities (ids n_plain .. n_plain + n - 1, none registered) beside `n_plain` registered plain actors.  Entity
    i gets a job every period_i ticks for `ticks` ticks (Workload.schedule, run_schedule), period_i drawn from 1, 2,
    idle, idle + 1, idle + 2 and 2 * idle + 3: the first two keep an entity busy, the last lets it passivate between
    two jobs, the ones between land in the ticks of the Idle, of the stop message and right after it.  An entity
    starts on its first job with the receive timeout `idle`; idle it receives Idle, passivates, stops on Bye, and its
    next job starts it again: state word 0 counts the jobs of the current incarnation.  With probability
    `p_passivate` / `p_stop` per entity and tick the host also sends Passivate (ignored while one is under way) or
    Stop (a plain stop: the mail queued behind it is dead letters).  The run goes quiescent once every entity has
    passivated after the last tick."""
    rng = np.random.default_rng(seed)
    periods = np.asarray([1, 2, idle, idle + 1, idle + 2, 2 * idle + 3], np.int64)
    per = periods[rng.integers(0, len(periods), n)]
    phase = rng.integers(0, 1 << 30, n) % per
    ids = (np.arange(n, dtype=np.uint32) + np.uint32(n_plain))
    schedule = []
    for t in range(ticks):
        ctl = rng.random(n)
        pas, stp = ids[ctl < p_passivate], ids[(ctl >= p_passivate) & (ctl < p_passivate + p_stop)]
        job = ids[(t % per) == phase]
        dst = np.concatenate([pas, stp, job, np.arange(n_plain, dtype=np.uint32)[: 1 if n_plain else 0]])
        pay = np.concatenate([np.full(pas.size, SE_PASSIVATE << 24, np.uint32), np.full(stp.size, SE_STOP << 24, np.uint32),
                              np.full(dst.size - pas.size - stp.size, SE_JOB << 24, np.uint32)])
        schedule.append((dst, np.full(dst.size, NO_SENDER, np.uint32), pay))
    return _sharded("sharded_entities", n, n_plain, idle, throughput, bucket_actors, schedule)


def passivation_race(n: int = 1 << 16, idle: int = 2, throughput: int = 16, bucket_actors: int = 256, n_plain: int = 8,
                     capacity: int = 0) -> Workload:
    """Jobs timed against the stop message.  Every entity starts on a job at tick 1, receives Idle at tick 1 + idle and
    passivates; its stop message arrives at tick S = 2 + idle.  By i mod 4 the host sends entity i a job for tick S
    (behind the stop message: buffered, the entity restarts), for tick S + 1 (the entity is gone: a fresh start), for
    both, or three jobs for tick S - 1, ahead of the Idle envelope -- at throughput 1 the envelope, and later the stop
    message, then wait behind them.  Run at throughput 1 and 16."""
    ids = (np.arange(n, dtype=np.uint32) + np.uint32(n_plain))
    c = np.arange(n) % 4
    S = 2 + idle
    at = {1: [ids], S - 1: [ids[c == 3]] * 3, S: [ids[(c == 0) | (c == 2)]], S + 1: [ids[(c == 1) | (c == 2)]]}
    schedule = []
    for t in range(1, S + 2):
        dst = np.concatenate(at.get(t, []) + [np.zeros(0, np.uint32)]).astype(np.uint32)
        schedule.append((dst, np.full(dst.size, NO_SENDER, np.uint32), np.full(dst.size, SE_JOB << 24, np.uint32)))
    return _sharded("passivation_race", n, n_plain, idle, throughput, bucket_actors, schedule, capacity)


# ------------------------------------------------------------------ the ask pattern: clients that bound their wait
AP_TICK, AP_REQUEST, AP_REPLY, AP_ANSWER, AP_TIMEOUT, AP_START = 1, 2, 3, 4, 5, 6
AP_TIMEOUT_UNIT = 1 << 32  # a client's word 0: answers in the low half, timeouts in the high half


def ask_client(timeout: int, period: int = 0, last_server: int | None = None):
    """A client (Behaviors.withTimers + context.ask): state word 0 counts answers (low half) and timeouts (high
    half), word 1 is the server it asks.  `period` > 0: every Tick of its periodic timer "tick" (key 0) it asks its
    server on key 1 (ask_pool).  `last_server` given: Start makes it ask; on a timeout it asks the next server, up to
    `last_server`, then counts the failure (ask_retry).  A reply comes back as Answer."""
    from . import typed
    B = typed.Behaviors
    tick, request, answer, timed_out, start = (typed.MessageType(n, t) for n, t in
                                               (("Tick", AP_TICK), ("Request", AP_REQUEST), ("Answer", AP_ANSWER),
                                                ("TimedOut", AP_TIMEOUT), ("Start", AP_START)))
    st = typed.State("count", "server")

    def ask(s):
        return typed.context.ask(s.server.ref, request(s.count), timeout, on_timeout=timed_out(), on_success=answer, key="ask")

    def build(timers):
        rb = typed.ReceiveBuilder.create(st)
        if period:
            timers.start_timer_with_fixed_delay("tick", tick(), period)  # (the setup start: Workload.timers["starts"])
            rb.on_message(tick, lambda m, s: [ask(s), B.same])
            rb.on_message(timed_out, lambda m, s: [s.count.add(AP_TIMEOUT_UNIT), B.same])
        else:
            rb.on_message(start, lambda m, s: [ask(s), B.same])
            rb.on_message(timed_out, lambda m, s: [s.server.inc(), ask(s), B.same], when=lambda m, s: s.server < last_server)
            rb.on_message(timed_out, lambda m, s: [s.count.add(AP_TIMEOUT_UNIT), B.same])
        return (rb.on_message(answer, lambda m, s: [s.count.inc(), B.same])
                .on_any_message(lambda m, s: [B.unhandled]).build("ask_client"))
    return B.with_timers(build)


def ask_server(silent: bool = False):
    """A server: counts the request and, unless `silent`, answers its sender -- the ask ref -- with Reply."""
    from . import typed
    B = typed.Behaviors
    request, reply = typed.MessageType("Request", AP_REQUEST), typed.MessageType("Reply", AP_REPLY)
    st = typed.State("served", "unused")
    rb = typed.ReceiveBuilder.create(st)
    if silent:
        rb.on_message(request, lambda m, s: [s.served.inc(), B.same])
    else:
        rb.on_message(request, lambda m, s: [s.served.inc(), m.sender.tell(reply(m.arg)), B.same])
    return rb.on_any_message(lambda m, s: [B.unhandled]).build("silent_server" if silent else "ask_server")


def _ask_servers(tb, loud, quiet, first: int, n_servers: int, silent_every: int) -> list:
    """The servers' ranges: every `silent_every`-th one (the last of each group) never answers; 0: all answer."""
    if not silent_every:
        return [(first, n_servers, tb.kind_of(loud), None)]
    ranges = []
    for j in range(0, n_servers, silent_every):
        g = min(silent_every, n_servers - j)
        if g == silent_every:
            if g > 1:
                ranges.append((first + j, g - 1, tb.kind_of(loud), None))
            ranges.append((first + j + g - 1, 1, tb.kind_of(quiet), None))
        else:
            ranges.append((first + j, g, tb.kind_of(loud), None))
    return ranges


def ask_pool(n_clients: int = 3 << 18, n_servers: int = 1 << 18, timeout: int = 4, silent_every: int = 8, period: int = 8,
             seed: int = 1, throughput: int = 4, bucket_actors: int = 0, asking: bool = True) -> Workload:
    """Clients (ids 0..n_clients-1) ask server n_clients + i mod n_servers every `period` ticks (a periodic Tick on
    key 0, staggered phases; the ask on key 1) and wait at most `timeout` ticks; every `silent_every`-th server never
    answers (0: all answer).  A client's word 0 counts its answers (low half) and timeouts (high half).  The
    periodic timers never let the engine go quiescent: run it with a budget.  A server bucket takes n_clients /
    n_servers / period requests per server and tick, well inside the timers engine's 2048-message tile at the default 2048-actor buckets
    (measured at 2^20 actors: 0.22 ms per tick there, 0.40 at 1024, 0.94 at 256: DESIGN.md §8 round 18).  `asking=False`: the same population on
    the same engine with no timer started, so nothing is ever asked -- what the instantiation costs at rest."""
    from . import typed
    rng = np.random.default_rng(seed)
    client, loud, quiet = ask_client(timeout, period=period), ask_server(), ask_server(silent=True)
    tb = typed.compile_behaviors([client, loud, quiet], max_emit=1)
    init = np.zeros((n_clients, 2), np.uint64)
    init[:, 1] = n_clients + np.arange(n_clients, dtype=np.uint64) % n_servers
    delays = (1 + rng.integers(0, period, n_clients)).astype(np.uint32)
    starts = [(0, n_clients, 0, True, period, delays, AP_TICK << 24)] if asking else []
    return Workload("ask_pool", n_clients + n_servers, 2, 1, throughput, 0,
                    [(0, n_clients, tb.kind_of(client), init)] + _ask_servers(tb, loud, quiet, n_clients, n_servers, silent_every),
                    behaviors=tb, bucket_actors=bucket_actors, timers={"n_keys": tb.timer_keys, "starts": starts, "ask": True})


def ask_retry(n_clients: int = 1 << 16, n_servers: int = 64, timeout: int = 3, silent_every: int = 2,
              throughput: int = 4, bucket_actors: int = 256) -> Workload:
    """Every client is told Start and asks server n_clients + i mod n_servers; on a timeout it asks the next server,
    and gives up (a counted timeout) past the last one.  Every `silent_every`-th server never answers.  The run goes
    quiescent once every client has its answer or has given up."""
    from . import typed
    last = n_clients + n_servers - 1
    client, loud, quiet = ask_client(timeout, last_server=last), ask_server(), ask_server(silent=True)
    tb = typed.compile_behaviors([client, loud, quiet], max_emit=1)
    init = np.zeros((n_clients, 2), np.uint64)
    init[:, 1] = n_clients + np.arange(n_clients, dtype=np.uint64) % n_servers
    ids = np.arange(n_clients, dtype=np.uint32)
    tells = (ids, np.full(n_clients, NO_SENDER, np.uint32), np.full(n_clients, AP_START << 24, np.uint32))
    return Workload("ask_retry", n_clients + n_servers, 2, 1, throughput, 0,
                    [(0, n_clients, tb.kind_of(client), init)] + _ask_servers(tb, loud, quiet, n_clients, n_servers, silent_every),
                    behaviors=tb, tells=tells, bucket_actors=bucket_actors,
                    timers={"n_keys": tb.timer_keys, "ask": True})


# ------------------------------------------------------------------ death watch: pacts and a self-healing ring
DW_STOP, DW_DOWN = 1, 2


def death_pact_chain(n: int = 1 << 20, throughput: int = 3, bucket_actors: int = 0) -> Workload:
    """Actor i watches actor i - 1 and handles no Terminated signal (the death pact, ActorAdapter.scala:200-205):
    a staged Stop to actor 0 takes the whole chain down, one actor every two ticks (a death at tick s reaches
    its watcher's inbox at s + 2), so every actor is dead after 2 n - 1 ticks."""
    from . import typed
    st = typed.State("count", "unused")
    B = typed.Behaviors
    b = (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [s.count.inc(), B.stopped], test=lambda m: m.tag == DW_STOP)
         .on_any_message(lambda m, s: [B.unhandled])
         .build("pact_link"))
    tb =typed.compile_behaviors([b], max_emit=1)
    tells = (np.asarray([0], np.uint32), np.asarray([NO_SENDER], np.uint32), np.asarray([DW_STOP << 24], np.uint32))
    return Workload("death_pact_chain", n, 2, 1, throughput, 0, [(0, n, tb.kind_of(b), None)], behaviors=tb, tells=tells,
                    bucket_actors=bucket_actors,
                    watch={"n_slots": 1, "starts": [(1, n - 1, None, -1, None)] if n > 1 else []})


def watch_ring(n: int = 1 << 20, kill=(0,), throughput: int = 3, bucket_actors: int = 0) -> Workload:
    """A ring that heals itself: every actor watchWith(Down)es its successor, held in a state word; on Down it
    counts the loss and watches the successor's successor -- a ref computed from state, possibly dead already
    (adjacent kills: answered one tick later), in the slot the Terminated has just freed.  `kill`: the actors that
    get a staged Stop."""
    from . import typed
    st = typed.State("succ", "downs")
    B = typed.Behaviors
    ctx = typed.context
    down = typed.MessageType("Down", DW_DOWN)
    b = (typed.ReceiveBuilder.create(st)
         .on_any_message(lambda m, s: [B.stopped], test=lambda m: m.tag == DW_STOP)
         .on_any_message(lambda m, s: [s.downs.inc(), s.succ.set(0), ctx.watch_with(s.succ.ref, down(0)), B.same],
                         test=lambda m: m.tag == DW_DOWN, when=lambda m, s: s.succ >= n - 1)
         .on_any_message(lambda m, s: [s.downs.inc(), s.succ.inc(), ctx.watch_with(s.succ.ref, down(0)), B.same],
                         test=lambda m: m.tag == DW_DOWN)
         .on_any_message(lambda m, s: [B.unhandled])
         .build("ring_member"))
    tb = typed.compile_behaviors([b], max_emit=1)
    init = np.zeros((n, 2), np.uint64)
    init[:, 0] = (np.arange(n, dtype=np.uint64) + 1) % n
    k = np.asarray(sorted(set(int(x) % n for x in kill)), np.uint32)
    tells = (k, np.full(k.size, NO_SENDER, np.uint32), np.full(k.size, DW_STOP << 24, np.uint32)) if k.size else None
    return Workload("watch_ring", n, 2, 1, throughput, 0, [(0, n, tb.kind_of(b), init)], behaviors=tb, tells=tells,
                    bucket_actors=bucket_actors,
                    watch={"n_slots": 1, "starts": [(0, n, None, 1, down.payload(0))]})


# ------------------------------------------------------------------ supervision: workers that fail and restart
FW_JOB, FW_POISON, FW_RESTARTED, FW_STOPPED = 1, 2, 3, 4


def flaky_workers(n: int = 1 << 20, hops: int = 8, poison_every: int = 16, max_poison: int = 5, max_restarts: int = 3,
                  within: int = 4, n_host: int = 4, seed: int = 1, throughput: int = 3, bucket_actors: int = 1024) -> Workload:
    """Workers under restart.with_limit(max_restarts, within) (TY/internal/Supervision.scala:311-406).  Every
    worker gets a Job(hops), counts it and passes it on with one hop less; one worker in `poison_every` also gets
    1..max_poison poison jobs, on each of which it throws.  A restart resets the jobs done since the last one
    (word 0) and keeps the worker's monitor (word 1, a host-side actor: a constructor argument); PreRestart reports
    the lost count to the monitor, and PostStop reports a worker that ran out of restarts and stopped -- the
    jobs that reach it afterwards are dead letters.  (Buckets of 1024 actors: the first tick's inbox of a bucket,
    a job per worker and the poison, stays within the one tile an engine with supervision handles.)"""
    from . import typed
    st = typed.State("since", "monitor")
    B = typed.Behaviors
    job = typed.MessageType("Job", FW_JOB)
    poisoned = typed.ExceptionType("PoisonedJob")
    b = (typed.ReceiveBuilder.create(st)
         .on_message(job, lambda m, s: [s.since.inc(), typed.self_ref(1).tell(job(m.arg - 1)), B.same], test=lambda m: m.arg > 0)
         .on_message(job, lambda m, s: [s.since.inc(), B.same])
         .on_any_message(lambda m, s: [B.throw(poisoned)], test=lambda m: m.tag == FW_POISON)
         .on_any_message(lambda m, s: [B.unhandled])
         .on_signal(typed.PreRestart, lambda sig, s: [s.monitor.ref.tell(s.since, tag=FW_RESTARTED), B.same])
         .on_signal(typed.PostStop, lambda sig, s: [s.monitor.ref.tell(s.since, tag=FW_STOPPED), B.same])
         .build("flaky_worker"))
    b = B.supervise(b, reset={st.since: 0}).on_failure(typed.SupervisorStrategy.restart.with_limit(max_restarts, within),
                                                       exc=poisoned)
    tb = typed.compile_behaviors([b], max_emit=1)
    rng = np.random.default_rng(seed)
    init = np.zeros((n, 2), np.uint64)
    init[:, 1] = n + np.arange(n, dtype=np.uint64) % max(n_host, 1)
    sick = np.flatnonzero(rng.random(n) < 1.0 / poison_every).astype(np.uint32)
    doses = rng.integers(1, max_poison + 1, sick.size)
    dst = np.concatenate([np.arange(n, dtype=np.uint32), np.repeat(sick, doses)])
    pay = np.concatenate([np.full(n, job.payload(hops), np.uint32), np.full(int(doses.sum()), FW_POISON << 24, np.uint32)])
    return Workload("flaky_workers", n, 2, 1, throughput, 0, [(0, n, tb.kind_of(b), init)], behaviors=tb,
                    tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), pay), outbound=(n, max(n_host, 1)),
                    bucket_actors=bucket_actors, supervision={"rows": tb.supervisors})


# ------------------------------------------------------------------ restartWithBackoff
BW_JOB, BW_RESTARTED, BW_STOPPED = 1, 3, 4


def backoff_workers(n: int = 1 << 20, jobs: int = 8, hops: int = 6, away_every: int = 8, max_away: int = 6,
                    min_backoff: int = 1, max_backoff: int = 16, random_factor: float = 0.2, reset_after: int = 4,
                    max_restarts: int = -1, stash_capacity: int = -1, seed: int = 1, throughput: int = 3,
                    bucket_actors: int = 128, churn: int = 0) -> Workload:
    """Flaky clients of a resource that is away for a stretch, under restart_with_backoff (TY/internal/Supervision.
    scala:163-406).  Every client gets `jobs` Job(hops) messages, counts each and passes it on with one hop less.
    One client in `away_every` finds its resource away for its next 1..max_away jobs (word 1, seeded; a constructor
    argument, so a restart keeps what is left of it): on each of them it throws ResourceAway, restarts and backs
    off -- 1, 2, 4, ... ticks with jitter, so with max_away > 3 the counts pass 3 -- while its other jobs and its
    neighbour's wait in the stash; once the resource is back it works them off in order.  (The resource is each
    client's own countdown and no actor of its own: a client that waits for a reply needs an ask timeout, and timers
    share no engine with supervision.)  PreRestart reports the jobs done since the last restart (word 0, which the
    restart resets) to the monitor, a host-side actor; PostStop reports a client that ran out of restarts.
    `churn` > 0 keeps the failures coming for as long as jobs circulate: every client also throws on the job after
    its `churn`-th since the last restart, passing that job on first."""
    from . import typed
    st = typed.State("since", "away")
    B = typed.Behaviors
    job = typed.MessageType("Job", BW_JOB)
    away = typed.ExceptionType("ResourceAway")
    monitor = typed.actor_ref(n)
    rb = typed.ReceiveBuilder.create(st)
    rb.on_message(job, lambda m, s: [s.away.add(-1), B.throw(away)], when=lambda m, s: s.away > 0)
    rb.on_message(job, lambda m, s: [s.since.inc(), B.same], test=lambda m: m.arg == 0)
    if churn:  # steady churn: the resource is away again for every `churn`-th job; that job is passed on before the throw
        rb.on_message(job, lambda m, s: [typed.self_ref(1).tell(job(m.arg - 1)), B.throw(away)], when=lambda m, s: s.since >= churn)
    rb.on_message(job, lambda m, s: [s.since.inc(), typed.self_ref(1).tell(job(m.arg - 1)), B.same])
    rb.on_any_message(lambda m, s: [B.unhandled])
    if not churn:  # (the passing-on throw takes the message's one tell: no reports then)
        rb.on_signal(typed.PreRestart, lambda sig, s: [monitor.tell(s.since, tag=BW_RESTARTED), B.same])
        rb.on_signal(typed.PostStop, lambda sig, s: [monitor.tell(s.since, tag=BW_STOPPED), B.same])
    b = rb.build("backoff_worker")
    strat = (typed.SupervisorStrategy.restart_with_backoff(min_backoff, max_backoff, random_factor)
             .with_max_restarts(max_restarts).with_reset_backoff_after(reset_after).with_stash_capacity(stash_capacity))
    b = B.supervise(b, reset={st.since: 0}).on_failure(strat, exc=away)
    tb = typed.compile_behaviors([b], max_emit=1)
    rng = np.random.default_rng(seed)
    init = np.zeros((n, 2), np.uint64)
    sick = np.flatnonzero(rng.random(n) < 1.0 / away_every)
    init[sick, 1] = rng.integers(1, max_away + 1, sick.size)
    dst = np.tile(np.arange(n, dtype=np.uint32), jobs)  # (round-robin: job j of every client before job j + 1 of any)
    pay = np.full(dst.size, job.payload(hops), np.uint32)
    return Workload("backoff_workers", n, 2, 1, throughput, 0, [(0, n, tb.kind_of(b), init)], behaviors=tb,
                    tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), pay), outbound=(n, 1),
                    bucket_actors=bucket_actors, supervision={"rows": tb.supervisors, "backoff": tb.backoff})


BS_TICK, BS_DATA, BS_RESTARTED = 1, 2, 3


def backoff_stash_pressure(n: int = 1 << 12, ticks: int = 24, poison_every: int = 6, capacities=(0, 1, 2, -1),
                           mailbox_capacity: int = 4, min_backoff: int = 2, max_backoff: int = 8, reset_after: int = 3,
                           seed: int = 1, bucket_actors: int = 64) -> Workload:
    """Steady senders against suspended actors with small stash capacities.  The first half of the actors are
    senders, the second half their targets (word 1 of a sender: a constructor argument).  Every sender starts with
    `ticks` Tick messages and drains one per tick (throughput 1), sending its target a Data message each time; one
    Data in `poison_every` (seeded) is poison, on which the target throws and backs off for 2, 4, 8 ticks.  While
    it is suspended a message a tick presses on a stash of capacities[k] (the targets take the capacities block by
    block; -1: the bounded mailbox's `mailbox_capacity`): what does not fit is dropped.  PreRestart reports the
    Data a target had counted (word 0, which the restart resets) to the monitor, a host-side actor."""
    from . import typed
    assert n % (2 * len(capacities)) == 0 and n >= 2 * len(capacities)
    assert ticks * bucket_actors <= 2048, "the start-up Ticks of a bucket stay within one tile"
    B = typed.Behaviors
    tick = typed.MessageType("Tick", BS_TICK)
    bad = typed.ExceptionType("PoisonedData")
    monitor = typed.actor_ref(n)
    sst = typed.State("sent", "target")
    sender = (typed.ReceiveBuilder.create(sst)
              .on_message(tick, lambda m, s: [s.sent.inc(), s.target.ref.tell(m.arg, tag=BS_DATA), B.same])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("pressure_sender"))
    behs = [sender]
    for k, cap in enumerate(capacities):
        tst = typed.State("got", "unused")
        t = (typed.ReceiveBuilder.create(tst)
             .on_any_message(lambda m, s: [B.throw(bad)], test=lambda m: m.tag == BS_DATA, when=lambda m, s: m.arg == 1)
             .on_any_message(lambda m, s: [s.got.inc(), B.same], test=lambda m: m.tag == BS_DATA)
             .on_any_message(lambda m, s: [B.unhandled])
             .on_signal(typed.PreRestart, lambda sig, s: [monitor.tell(s.got, tag=BS_RESTARTED), B.same])
             .build(f"pressure_target_{k}"))
        strat = (typed.SupervisorStrategy.restart_with_backoff(min_backoff, max_backoff, 0.0)
                 .with_reset_backoff_after(reset_after).with_stash_capacity(cap))
        behs.append(B.supervise(t, reset={tst.got: 0}).on_failure(strat, exc=bad))
    tb = typed.compile_behaviors(behs, max_emit=1)
    h, blk = n // 2, n // 2 // len(capacities)
    init = np.zeros((h, 2), np.uint64)
    init[:, 1] = h + np.arange(h, dtype=np.uint64)
    ranges = [(0, h, tb.kind_of(sender), init)]
    ranges += [(h + k * blk, blk, tb.kind_of(behs[1 + k]), None) for k in range(len(capacities))]
    rng = np.random.default_rng(seed)
    dst = np.tile(np.arange(h, dtype=np.uint32), ticks)
    pay = ((BS_TICK << 24) | (rng.random(dst.size) < 1.0 / poison_every)).astype(np.uint32)
    # (the targets' bounded mailbox is class 1; the senders' start-up Ticks need the unbounded default)
    return Workload("backoff_stash_pressure", n, 2, 1, 1, 0, ranges, behaviors=tb,
                    tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), pay), outbound=(n, 1),
                    bucket_actors=bucket_actors, mailbox_classes={1: mailbox_capacity}, mailboxes=[(h, h, 1)],
                    supervision={"rows": tb.supervisors, "backoff": tb.backoff})


# ------------------------------------------------------------------ children
CH_SPAWN, CH_STOP, CH_WORK = 1, 2, 3


def spawn_tree_levels(depth: int, fanout: int) -> list:
    """(first id, count) of every level of spawn_tree(depth, fanout), the root first."""
    out, first = [], 0
    for lv in range(depth + 1):
        out.append((first, fanout ** lv))
        first += fanout ** lv
    return out


def spawn_tree(depth: int = 4, fanout: int = 32, throughput: int = 3, bucket_actors: int = 0) -> Workload:
    """A tree that grows on the device, level by level (at most 8 levels below the root: one region each).  Only
    the root is registered.  A node holds its remaining depth in state word 0 and its parent in word 1; on Spawn
    it spawns one child with depth - 1 while its depth is above 0 (a leaf leaves Spawn unhandled), on Stop it stops.
    With max_emit = 1 a message has one envelope to send and the Create takes it, so the host tells every node of
    a level `fanout` Spawn messages (grow_tree) instead of the nodes telling each other.  Stopping the root then
    takes the tree down one level per tick."""
    from . import typed
    if not 1 <= depth <= 8:
        raise ValueError("spawn_tree: depth 1..8 (one region per level)")
    st = typed.State("depth", "parent")
    B, ctx = typed.Behaviors, typed.context
    node = typed.Behavior("tree_node", st)
    (typed.ReceiveBuilder.create(st)
     .on_any_message(lambda m, s: [ctx.spawn(node, arg=s.depth - 1, word1=ctx.PARENT), B.same],
                     test=lambda m: m.tag == CH_SPAWN, when=lambda m, s: s.depth > 0)
     .on_any_message(lambda m, s: [B.stopped], test=lambda m: m.tag == CH_STOP)
     .on_any_message(lambda m, s: [B.unhandled])
     .build(into=node))
    tb = typed.compile_behaviors([node], max_emit=1)
    lv = spawn_tree_levels(depth, fanout)
    regions = [(lv[i][0], lv[i][1], lv[i + 1][0], fanout) for i in range(depth)]
    n = lv[-1][0] + lv[-1][1]
    return Workload("spawn_tree", n, 2, 1, throughput, 0,
                    [(0, 1, tb.kind_of(node), np.asarray([[depth, 0xFFFFFFFF]], np.uint64))], behaviors=tb,
                    bucket_actors=bucket_actors, watch={"n_slots": 1},
                    children={"regions": regions, "sites": tb.spawn_sites})


def grow_tree(target, depth: int, fanout: int, run=None):
    """Grow spawn_tree(depth, fanout) on `target`: per level, `fanout` Spawn messages to each of its nodes, then a
    run to quiescence; -> the stats of every run (`run(target)` replaces target.run())."""
    out = []
    for first, count in spawn_tree_levels(depth, fanout)[:-1]:
        dst = np.repeat(np.arange(first, first + count, dtype=np.uint32), fanout)
        target.tell(dst, np.full(dst.size, CH_SPAWN << 24, np.uint32), np.full(dst.size, NO_SENDER, np.uint32))
        out.append(target.run() if run is None else run(target))
    return out


def pool_router(n_routers: int = 1 << 14, pool_size: int = 16, throughput: int = 3, bucket_actors: int = 0,
                host_id: int | None = None) -> Workload:
    """Routers.pool(pool_size) with round-robin logic (PoolRouterImpl.scala:60-64, RoutingLogic.scala:42-53):
    router r (ids 0..n_routers - 1) spawns its routees in the setup block (ids n_routers + r * pool_size + k),
    watches them and forwards every Work message to child number `next`, then next += 1.  It stops when its last
    routee has (RoutersSpec.scala:104): it counts the Terminated signals.  An actor has at most four watch slots,
    so a router watches its first four routees (pool_watch_starts) and, at every Terminated, the next one not yet
    watched; one that is dead already answers a tick later.  A routee counts its Work, keeps the last payload
    (and echoes it to `host_id` when given) and stops on Stop."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    rs = typed.State("count", "last")
    echo = (lambda m: [typed.actor_ref(host_id).tell(m.payload)]) if host_id is not None else (lambda m: [])
    routee = (typed.ReceiveBuilder.create(rs)
              .on_any_message(lambda m, s: [B.stopped], test=lambda m: m.tag == CH_STOP)
              .on_any_message(lambda m, s: [s.count.inc(), s.last.set(m.payload)] + echo(m) + [B.same],
                              test=lambda m: m.tag == CH_WORK)
              .on_any_message(lambda m, s: [B.unhandled])
              .build("routee"))
    st = typed.State("next", "dead")
    slots = min(pool_size, typed.MAX_WATCH_SLOTS)
    router = typed.Behavior("pool_router", st)
    setup = ctx.spawn(routee, word1=ctx.PARENT)  # the setup block's spawn: its site is site 0 (agx_spawn_children)
    (typed.ReceiveBuilder.create(st)
     .on_any_message(lambda m, s: [ctx.child_at(s.next).tell(m.payload), s.next.inc(), B.same], test=lambda m: m.tag == CH_WORK)
     .on_any_message(lambda m, s: [setup, B.same], test=lambda m: m.tag == CH_SPAWN)
     .on_any_message(lambda m, s: [B.unhandled])
     .on_signal(typed.Terminated, lambda sig, s: [s.dead.inc(), B.stopped], when=lambda sig, s: s.dead + 1 >= pool_size)
     .on_signal(typed.Terminated, lambda sig, s: [s.dead.inc(), ctx.watch(ctx.child_at(s.dead + (slots - 1))), B.same],
                when=lambda sig, s: s.dead + slots < pool_size)
     .on_signal(typed.Terminated, lambda sig, s: [s.dead.inc(), B.same])
     .build(into=router))
    tb = typed.compile_behaviors([router], max_emit=1)
    n = n_routers * (1 + pool_size)
    return Workload("pool_router", n, 2, 1, throughput, 0, [(0, n_routers, tb.kind_of(router), None)], behaviors=tb,
                    bucket_actors=bucket_actors, outbound=(host_id, 1) if host_id is not None else None,
                    watch={"n_slots": slots, "starts": pool_watch_starts(n_routers, pool_size)},
                    children={"regions": [(0, n_routers, n_routers, pool_size)], "sites": tb.spawn_sites,
                              "spawns": [(0, n_routers, 0, 0)] * pool_size})


def pool_watch_starts(n_routers: int, pool_size: int) -> list:
    """pool_router's setup watches: router r watches its routees 0 .. min(pool_size, 4) - 1."""
    r = np.arange(n_routers, dtype=np.uint32)
    return [(0, n_routers, n_routers + r * pool_size + k, 0, None) for k in range(min(pool_size, 4))]


# ------------------------------------------------------------------ the receptionist and group routers
SP_JOB = 1
SM_REG, SM_DEREG, SM_STOP, SM_ROUTE, SM_ROUTE_BY, SM_FIND, SM_WORK, SM_SIZE = 1, 2, 3, 4, 5, 6, 7, 8


def service_pool(n_routers: int = 1 << 10, n_workers: int = 1 << 14, ticks: int = 16, quota: int = 0, throughput: int = 3,
                 bucket_actors: int = 0, n_host: int = 0) -> Workload:
    """Routers.group(key) with round-robin logic over workers that come and go (GroupRouterImpl.scala:114-146,
    RoutingLogic.scala:42-75): the workers (ids n_routers ..) register in the setup block, every router (ids 0 ..
    n_routers - 1) gets one Job per tick from the host schedule and forwards it to the next registered worker; the
    routers' cursors start spread over the workers, so a tick's jobs spread too.  A worker counts its jobs and keeps
    the last payload (with n_host > 0 it answers the job's sender, the forward's replyTo); with `quota` > 0 worker i
    stops after 1 + i mod quota jobs, so the listing shrinks tick by tick; with quota 0 the listing is stable."""
    from . import typed
    B = typed.Behaviors
    key = typed.ServiceKey("worker")
    job = typed.MessageType("Job", SP_JOB)
    router = typed.Routers.group(key).with_round_robin_routing().build("group_router")
    ws = typed.State("left", "last")
    done = lambda m, s: [s.left.add(-1), s.last.set(m.payload)] + ([m.sender.tell(m.payload)] if n_host else [])
    worker = (typed.ReceiveBuilder.create(ws)
              .on_message(job, lambda m, s: done(m, s) + [B.stopped], when=lambda m, s: s.left == 1)
              .on_message(job, lambda m, s: done(m, s) + [B.same])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("pool_worker"))
    tb = typed.compile_behaviors([router, worker], max_emit=1)
    n = n_routers + n_workers
    r = np.arange(n_routers, dtype=np.uint64)
    rinit = np.zeros((n_routers, 2), np.uint64)
    rinit[:, 0] = n_routers + r * n_workers // max(n_routers, 1)
    winit = np.zeros((n_workers, 2), np.uint64)
    winit[:, 0] = 1 + np.arange(n_workers, dtype=np.uint64) % quota if quota else 0  # (0: never reaches 1 going down)
    dst = np.arange(n_routers, dtype=np.uint32)
    src = (n + dst % n_host).astype(np.uint32) if n_host else np.full(n_routers, NO_SENDER, np.uint32)
    schedule = [(dst, src, np.full(n_routers, job.payload(t + 1), np.uint32)) for t in range(ticks)]
    return Workload("service_pool", n, 2, 1, throughput, 0,
                    [(0, n_routers, tb.kind_of(router), rinit), (n_routers, n_workers, tb.kind_of(worker), winit)],
                    behaviors=tb, bucket_actors=bucket_actors, outbound=(n, n_host) if n_host else None,
                    receptionist={"n_keys": 1, "capacity": n_workers, "starts": [(n_routers, n_workers, 0)]},
                    schedule=schedule)


# ------------------------------------------------------------------ consistent-hashing and random routing
SS_TICK, SS_REQUEST, SS_JOIN = 1, 2, 3


def sticky_sessions(n_clients: int = 1 << 12, n_routers: int = 64, n_workers: int = 1 << 10, n_spare: int = 0, quota: int = 0,
                    virtual_nodes_factor: int = 10, ticks: int = 16, join_at: int = 0, seed: int = 1, throughput: int = 3,
                    bucket_actors: int = 0) -> Workload:
    """Sticky sessions over a changing worker pool (Routers.group(key).withConsistentHashingRouting, RoutingLogic.scala:
    93-112): client c (ids 0 ..) holds a session number and, on every Tick of the host schedule, sends Request(session)
    to router c mod n_routers (ids n_clients ..), a group router with consistent-hashing logic keyed by the session; the
    worker (ids n_clients + n_routers ..) counts down `left` and keeps the last session it served.  The first n_workers
    - n_spare workers register in the setup block; with `quota` > 0 worker i stops after 1 + i mod quota requests, so
    ring points leave tick by tick; the n_spare last workers register when the host's Join reaches them before tick
    `join_at` + 1.  A session stays with its worker while that worker is registered."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    key = typed.ServiceKey("session_worker")
    tick, request, join = (typed.MessageType("Tick", SS_TICK), typed.MessageType("Request", SS_REQUEST),
                           typed.MessageType("Join", SS_JOIN))
    cs = typed.State("session", "router")
    client = (typed.ReceiveBuilder.create(cs)
              .on_message(tick, lambda m, s: [typed.Ref(s.router).tell(request(s.session)), B.same])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("session_client"))
    router = typed.Routers.group(key).with_consistent_hash_routing(virtual_nodes_factor, lambda m: m.arg).build("hash_router")
    ws = typed.State("left", "last")
    worker = (typed.ReceiveBuilder.create(ws)
              .on_message(request, lambda m, s: [s.left.add(-1), s.last.set(m.arg), B.stopped], when=lambda m, s: s.left == 1)
              .on_message(request, lambda m, s: [s.left.add(-1), s.last.set(m.arg), B.same])
              .on_message(join, lambda m, s: [ctx.register(key), B.same])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("session_worker"))
    tb = typed.compile_behaviors([client, router, worker], max_emit=1)
    n = n_clients + n_routers + n_workers
    c = np.arange(n_clients, dtype=np.uint64)
    cinit = np.zeros((n_clients, 2), np.uint64)
    cinit[:, 0] = splitmix64_np(c + np.uint64(seed)) & np.uint64(0xFFFFFF)
    cinit[:, 1] = n_clients + c % max(n_routers, 1)
    winit = np.zeros((n_workers, 2), np.uint64)
    winit[:, 0] = 1 + np.arange(n_workers, dtype=np.uint64) % quota if quota else 0  # (0: never reaches 1 going down)
    w0 = n_clients + n_routers
    dst = np.arange(n_clients, dtype=np.uint32)
    none = np.full(n_clients, NO_SENDER, np.uint32)
    schedule = []
    for t in range(ticks):
        d, sr, py = dst, none, np.full(n_clients, tick.payload(t + 1), np.uint32)
        if n_spare and t == join_at:
            jd = np.arange(w0 + n_workers - n_spare, w0 + n_workers, dtype=np.uint32)
            d = np.concatenate([d, jd])
            sr = np.concatenate([sr, np.full(n_spare, NO_SENDER, np.uint32)])
            py = np.concatenate([py, np.full(n_spare, join.payload(), np.uint32)])
        schedule.append((d, sr, py))
    return Workload("sticky_sessions", n, 2, 1, throughput, 0,
                    [(0, n_clients, tb.kind_of(client), cinit), (n_clients, n_routers, tb.kind_of(router), None),
                     (w0, n_workers, tb.kind_of(worker), winit)],
                    behaviors=tb, bucket_actors=bucket_actors,
                    receptionist={"n_keys": 1, "capacity": n_workers, "starts": [(w0, n_workers - n_spare, 0)]},
                    router_logics={"hashed_keys_mask": tb.hashed_keys_mask, "virtual_nodes_factor": tb.virtual_nodes_factor,
                                   "seed": seed},
                    schedule=schedule)


def random_pool(n_routers: int = 1 << 10, n_workers: int = 1 << 14, ticks: int = 16, quota: int = 0, seed: int = 1,
                throughput: int = 3, bucket_actors: int = 0) -> Workload:
    """service_pool with Routers.group(key).withRandomRouting (RoutingLogic.scala:77-91): every router gets one Job per
    tick and forwards it to a worker drawn from the listing in force; with `quota` > 0 worker i stops after 1 + i mod
    quota jobs, so the listing shrinks tick by tick."""
    from . import typed
    B = typed.Behaviors
    key = typed.ServiceKey("worker")
    job = typed.MessageType("Job", SP_JOB)
    router = typed.Routers.group(key).with_random_routing().build("random_router")
    ws = typed.State("left", "last")
    done = lambda m, s: [s.left.add(-1), s.last.set(m.payload)]
    worker = (typed.ReceiveBuilder.create(ws)
              .on_message(job, lambda m, s: done(m, s) + [B.stopped], when=lambda m, s: s.left == 1)
              .on_message(job, lambda m, s: done(m, s) + [B.same])
              .on_any_message(lambda m, s: [B.unhandled])
              .build("pool_worker"))
    tb = typed.compile_behaviors([router, worker], max_emit=1)
    n = n_routers + n_workers
    winit = np.zeros((n_workers, 2), np.uint64)
    winit[:, 0] = 1 + np.arange(n_workers, dtype=np.uint64) % quota if quota else 0  # (0: never reaches 1 going down)
    dst = np.arange(n_routers, dtype=np.uint32)
    src = np.full(n_routers, NO_SENDER, np.uint32)
    schedule = [(dst, src, np.full(n_routers, job.payload(t + 1), np.uint32)) for t in range(ticks)]
    return Workload("random_pool", n, 2, 1, throughput, 0,
                    [(0, n_routers, tb.kind_of(router), None), (n_routers, n_workers, tb.kind_of(worker), winit)],
                    behaviors=tb, bucket_actors=bucket_actors,
                    receptionist={"n_keys": 1, "capacity": n_workers, "starts": [(n_routers, n_workers, 0)]},
                    router_logics={"hashed_keys_mask": 0, "seed": seed}, schedule=schedule)


def service_mesh(n: int = 4096, n_keys: int = 8, seed: int = 1, ticks: int = 40, throughput: int = 3, capacity: int = 16,
                 bucket_actors: int = 64, n_host: int = 4) -> Workload:
    """The differential workload of the receptionist: every actor runs one behaviour that, on host messages, registers
    under or deregisters from key (arg mod n_keys), stops, routes a Work message round robin (cursor: state word 0) or
    by index (its count, state word 1), finds a service (service_at) and tells it, or reports a listing's size to the
    message's sender; Work counts.  The host schedule draws, per tick, random actors for each of these (registrations
    outnumber stops, so listings grow, churn and shrink); a quarter of the actors are registered in the setup block.
    Bounded mailboxes (`capacity`) keep a popular routee's backlog, and so its bucket's inbox, within one tile."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    keys = [typed.ServiceKey(f"svc{k}") for k in range(n_keys)]
    st = typed.State("cursor", "count")
    work = typed.MessageType("Work", SM_WORK)
    rb = typed.ReceiveBuilder.create(st)
    tag = lambda t: (lambda m: m.tag == t)
    rb.on_any_message(lambda m, s: [s.count.inc(), B.stopped], test=tag(SM_STOP))
    rb.on_any_message(lambda m, s: [s.count.inc(), B.same], test=tag(SM_WORK))
    for k, key in enumerate(keys):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda key: lambda m, s: [ctx.register(key), B.same])(key), test=tag(SM_REG), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.deregister(key), B.same])(key), test=tag(SM_DEREG), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.route(key, work(s.count), cursor=s.cursor, forward=False), B.same])(key),
                          test=tag(SM_ROUTE), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.route_by(key, s.count, work(m.arg)), s.count.inc(), B.same])(key),
                          test=tag(SM_ROUTE_BY), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.service_at(key, s.cursor + 1).tell(work(1)), B.same])(key),
                          test=tag(SM_FIND), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [m.sender.tell(ctx.listing_size(key)), B.same])(key),
                          test=tag(SM_SIZE), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    node = rb.build("mesh_node")
    tb = typed.compile_behaviors([node], max_emit=1)
    rng = np.random.default_rng(seed)
    init = np.zeros((n, 2), np.uint64)
    init[:, 0] = rng.integers(0, n, n)
    schedule = []
    per = {SM_REG: n // 16, SM_DEREG: n // 32, SM_STOP: n // 128, SM_ROUTE: n // 16, SM_ROUTE_BY: n // 32, SM_FIND: n // 32,
           SM_SIZE: max(n // 256, 1)}
    for t in range(ticks):
        dst, pay = [], []
        for tg, cnt in per.items():
            if tg == SM_REG and t >= ticks * 3 // 4:  # (the tail: listings only shrink)
                continue
            d = rng.integers(0, n, cnt)
            dst.append(d)
            pay.append((tg << 24) | rng.integers(0, n_keys, cnt))
        dst = np.concatenate(dst).astype(np.uint32)
        o = rng.permutation(dst.size)
        src = (n + rng.integers(0, max(n_host, 1), dst.size)).astype(np.uint32)
        schedule.append((dst[o], src[o], np.concatenate(pay).astype(np.uint32)[o]))
    starts = [(int(f), int(n // (4 * n_keys)), k) for k, f in enumerate(rng.integers(0, n - n // (4 * n_keys), n_keys))]
    return Workload("service_mesh", n, 2, 1, throughput, capacity, [(0, n, tb.kind_of(node), init)], behaviors=tb,
                    bucket_actors=bucket_actors, outbound=(n, max(n_host, 1)),
                    receptionist={"n_keys": n_keys, "capacity": n, "starts": starts}, schedule=schedule)


# ------------------------------------------------------------------ pub-sub topics
TB_TICK, TB_NOTE = 1, 2
TM_SUB, TM_UNSUB, TM_STOP, TM_PUB, TM_COUNT, TM_NOTE, TM_SUBPUB, TM_PUBUNSUB = 1, 2, 3, 4, 5, 6, 7, 8


def topic_broadcast(n_publishers: int = 1, n_subscribers: int = 1 << 14, n_topics: int = 1, period: int = 1, ticks: int = 16,
                    throughput: int = 3, bucket_actors: int = 0, log_capacity: int = 1024) -> Workload:
    """Topic broadcast (TopicImpl.scala:60-143): publisher p (ids 0 .. n_publishers - 1) publishes Note(t) to topic
    p mod n_topics whenever the host schedule ticks it, every `period`-th tick; the subscribers (ids n_publishers ..)
    are subscribed in the setup block, the k-th block of n_subscribers / n_topics ids to topic k; a subscriber counts
    what it receives (state word 0) and sums the arguments (state word 1).  One publication then becomes n_subscribers / n_topics envelopes in the next tick."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    topics = [typed.Topic(f"topic{k}") for k in range(n_topics)]
    tick, note = typed.MessageType("Tick", TB_TICK), typed.MessageType("Note", TB_NOTE)
    ps = typed.State("sent", "topic")
    rb = typed.ReceiveBuilder.create(ps)
    for k, tp in enumerate(topics):
        rb.on_message(tick, (lambda tp: lambda m, s: [s.sent.inc(), ctx.publish(tp, note(m.arg)), B.same])(tp),
                      when=(lambda k: lambda m, s: s.topic == k)(k))
    rb.on_any_message(lambda m, s: [B.unhandled])
    publisher = rb.build("topic_publisher")
    ss = typed.State("count", "sum")
    subscriber = (typed.ReceiveBuilder.create(ss)
                  .on_message(note, lambda m, s: [s.count.inc(), s.sum.add(m.arg), B.same])
                  .on_any_message(lambda m, s: [B.unhandled])
                  .build("topic_subscriber"))
    tb = typed.compile_behaviors([publisher, subscriber], max_emit=1)
    n = n_publishers + n_subscribers
    pinit = np.zeros((n_publishers, 2), np.uint64)
    pinit[:, 1] = np.arange(n_publishers, dtype=np.uint64) % n_topics
    dst = np.arange(n_publishers, dtype=np.uint32)
    none = np.zeros(0, np.uint32)
    schedule = [(dst, np.full(n_publishers, NO_SENDER, np.uint32), np.full(n_publishers, tick.payload(t + 1), np.uint32))
                if t % period == 0 else (none, none, none) for t in range(ticks)]
    per = n_subscribers // n_topics
    starts = [(n_publishers + k * per, per if k < n_topics - 1 else n_subscribers - k * per, k) for k in range(n_topics)]
    return Workload("topic_broadcast", n, 2, 1, throughput, 0,
                    [(0, n_publishers, tb.kind_of(publisher), pinit), (n_publishers, n_subscribers, tb.kind_of(subscriber), None)],
                    behaviors=tb, bucket_actors=bucket_actors,
                    receptionist={"n_keys": n_topics, "capacity": n_subscribers, "starts": starts},
                    topics={"log_capacity": log_capacity}, schedule=schedule)


def topic_mesh(n: int = 1024, n_keys: int = 8, seed: int = 1, ticks: int = 40, throughput: int = 3, capacity: int = 4,
               bucket_actors: int = 64, n_host: int = 4, log_capacity: int = 1024) -> Workload:
    """The differential workload of the topics: every actor runs one behaviour that, on host messages, subscribes to
    or unsubscribes from topic (arg mod n_keys), stops, publishes Note(its count) to the topic, subscribes and
    publishes or publishes and unsubscribes in one case, or reports the topic's subscriber count to the message's
    sender; a Note is counted (state word 0) and its payload kept (state word 1: order-sensitive).  The host schedule
    draws, per tick, random actors for each of these; a few actors are subscribed in the setup block, and topic
    n_keys - 1 is only ever published to, so some publications find no subscriber.  Bounded mailboxes (`capacity`)
    turn the deliveries past a subscriber's capacity into dead letters and keep a bucket's inbox within one tile."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    topics = [typed.Topic(f"mesh{k}") for k in range(n_keys)]
    st = typed.State("count", "last")
    note = typed.MessageType("Note", TM_NOTE)
    rb = typed.ReceiveBuilder.create(st)
    tag = lambda t: (lambda m: m.tag == t)
    rb.on_any_message(lambda m, s: [s.count.inc(), B.stopped], test=tag(TM_STOP))
    rb.on_any_message(lambda m, s: [s.count.inc(), s.last.set(m.payload), B.same], test=tag(TM_NOTE))
    for k, tp in enumerate(topics):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.subscribe(tp), B.same])(tp), test=tag(TM_SUB), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.unsubscribe(tp), B.same])(tp), test=tag(TM_UNSUB), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.publish(tp, note(s.count)), B.same])(tp), test=tag(TM_PUB), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.subscribe(tp), ctx.publish(tp, note(s.count + 1)), B.same])(tp),
                          test=tag(TM_SUBPUB), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.publish(tp, note(s.count + 2)), ctx.unsubscribe(tp), B.same])(tp),
                          test=tag(TM_PUBUNSUB), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [m.sender.tell(ctx.subscriber_count(tp)), B.same])(tp),
                          test=tag(TM_COUNT), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    node = rb.build("topic_mesh_node")
    tb = typed.compile_behaviors([node], max_emit=1)
    rng = np.random.default_rng(seed)
    nsub = max(n_keys - 1, 1)  # (the last topic has no subscriber)
    per = {TM_SUB: max(n // 64, 1), TM_UNSUB: max(n // 128, 1), TM_STOP: max(n // 256, 1), TM_PUB: max(n // 256, 2),
           TM_SUBPUB: 1, TM_PUBUNSUB: 1, TM_COUNT: max(n // 256, 1)}
    schedule = []
    for t in range(ticks):
        dst, pay = [], []
        for tg, cnt in per.items():
            if tg == TM_SUB and t >= ticks * 3 // 4:  # (the tail: the topics only lose subscribers)
                continue
            d = rng.integers(0, n, cnt)
            dst.append(d)
            keys = rng.integers(0, n_keys if tg == TM_PUB else nsub, cnt)
            pay.append((tg << 24) | keys)
        dst = np.concatenate(dst).astype(np.uint32)
        o = rng.permutation(dst.size)
        src = (n + rng.integers(0, max(n_host, 1), dst.size)).astype(np.uint32)
        schedule.append((dst[o], src[o], np.concatenate(pay).astype(np.uint32)[o]))
    cnt0 = max(n // (16 * n_keys), 1)
    starts = [(int(f), cnt0, k) for k, f in enumerate(rng.integers(0, n - cnt0, nsub))]
    return Workload("topic_mesh", n, 2, 1, throughput, capacity, [(0, n, tb.kind_of(node), None)], behaviors=tb,
                    bucket_actors=bucket_actors, outbound=(n, max(n_host, 1)),
                    receptionist={"n_keys": n_keys, "capacity": n, "starts": starts},
                    topics={"log_capacity": log_capacity}, schedule=schedule)


# ------------------------------------------------------------------ Subscribe / Listing
SW_LISTING, SW_STOP, SW_DEREG, SW_REG = 1, 2, 3, 4
DW_LISTING, DW_GO, DW_JOB, DW_STOP = 1, 2, 3, 4


def service_watchers(n_services: int = 64, n_watchers: int = 1 << 14, ticks: int = 16, period: int = 1, throughput: int = 3,
                     bucket_actors: int = 0, stop: bool = False) -> Workload:
    """Watchers of one service key (LocalReceptionist.scala:152-166,213-220): the services (ids 0 .. n_services - 1)
    are registered and the watchers (ids n_services ..) subscribed in the setup block; a watcher keeps the size of
    the listing it was told last (state word 1) and counts its Listings (state word 0).  Every `period`-th tick the
    host tells one service to leave -- Deregister, or a stop with `stop` --, service t mod n_services in turn (a
    service that has left registers again when it is told a second time), so one key changes per such tick and
    every watcher receives one Listing in the tick after."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    key = typed.ServiceKey("watched")
    listing = typed.MessageType("Listing", SW_LISTING)
    leave, stopm = typed.MessageType("Leave", SW_DEREG), typed.MessageType("Stop", SW_STOP)
    ss = typed.State("told", "member")
    service = (typed.ReceiveBuilder.create(ss)
               .on_message(stopm, lambda m, s: [B.stopped])
               .on_message(leave, lambda m, s: [s.told.inc(), s.member.set(0), ctx.deregister(key), B.same], when=lambda m, s: s.member == 1)
               .on_message(leave, lambda m, s: [s.told.inc(), s.member.set(1), ctx.register(key), B.same])
               .on_any_message(lambda m, s: [B.unhandled])
               .build("watched_service"))
    ws = typed.State("listings", "size")
    watcher = (typed.ReceiveBuilder.create(ws)
               .on_message(listing, lambda m, s: [s.listings.inc(), s.size.set(ctx.listing_size(key)), B.same])
               .on_message(typed.MessageType("Subscribe", SW_REG), lambda m, s: [ctx.receptionist_subscribe(key, listing), B.same])
               .on_any_message(lambda m, s: [B.unhandled])
               .build("service_watcher"))
    tb = typed.compile_behaviors([service, watcher], max_emit=1)
    n = n_services + n_watchers
    sinit = np.zeros((n_services, 2), np.uint64)
    sinit[:, 1] = 1
    none = np.zeros(0, np.uint32)
    schedule = []
    for t in range(ticks):
        if t % period:
            schedule.append((none, none, none))
            continue
        who = (t // period) % n_services
        msg = stopm if stop else leave
        schedule.append((np.asarray([who], np.uint32), np.asarray([NO_SENDER], np.uint32), np.asarray([msg.payload()], np.uint32)))
    return Workload("service_watchers", n, 2, 1, throughput, 0,
                    [(0, n_services, tb.kind_of(service), sinit), (n_services, n_watchers, tb.kind_of(watcher), None)],
                    behaviors=tb, bucket_actors=bucket_actors,
                    receptionist={"n_keys": 1, "capacity": n_services, "starts": [(0, n_services, 0)]},
                    topics={"log_capacity": 1},
                    listings={"payloads": tb.listing_payloads, "starts": [(n_services, n_watchers, 0)]}, schedule=schedule)


def discovery_workers(n_services: int = 16, n_workers: int = 1 << 10, jobs: int = 4, throughput: int = 3,
                      bucket_actors: int = 0) -> Workload:
    """Wait for the first listing (the pattern the group router's initial stash stands for; GroupRouterImpl.scala:
    114-146, LocalReceptionist.scala:168-171,209-211): a worker told Go(x) finds the key and keeps x (state word 1);
    when the Listing arrives it sends Job(x) to service_at(x) and counts it (state word 0), `jobs` times over: with
    each job it finds the key again, and the next Listing brings the next job.  The services (ids 0 .. n_services - 1) are registered in the setup block and count
    their jobs (state word 0) and sum the arguments (state word 1).  The host tells every worker Go once."""
    from . import typed
    B, ctx = typed.Behaviors, typed.context
    key = typed.ServiceKey("workers_service")
    listing, go, job = (typed.MessageType("Listing", DW_LISTING), typed.MessageType("Go", DW_GO), typed.MessageType("Job", DW_JOB))
    ss = typed.State("jobs", "sum")
    service = (typed.ReceiveBuilder.create(ss)
               .on_message(job, lambda m, s: [s.jobs.inc(), s.sum.add(m.arg), B.same])
               .on_any_message(lambda m, s: [B.unhandled])
               .build("discovered_service"))
    ws = typed.State("sent", "x")
    rb = typed.ReceiveBuilder.create(ws)
    rb.on_message(go, lambda m, s: [s.x.set(m.arg), ctx.receptionist_find(key, listing), B.same])
    # the Listing, and then every job's own echo: send the next job while any is left
    rb.on_message(listing, lambda m, s: [s.sent.inc(), ctx.service_at(key, s.x).tell(job(s.x)), ctx.receptionist_find(key, listing), B.same],
                  when=lambda m, s: s.sent < jobs)
    rb.on_message(listing, lambda m, s: [B.same])
    rb.on_any_message(lambda m, s: [B.unhandled])
    worker = rb.build("discovery_worker")
    tb = typed.compile_behaviors([service, worker], max_emit=1)
    n = n_services + n_workers
    dst = np.arange(n_services, n, dtype=np.uint32)
    pay = ((DW_GO << 24) | (np.arange(n_workers, dtype=np.uint32) & 0xFFFFFF)).astype(np.uint32)
    schedule = [(dst, np.full(n_workers, NO_SENDER, np.uint32), pay)]
    return Workload("discovery_workers", n, 2, 1, throughput, 0,
                    [(0, n_services, tb.kind_of(service), None), (n_services, n_workers, tb.kind_of(worker), None)],
                    behaviors=tb, bucket_actors=bucket_actors,
                    receptionist={"n_keys": 1, "capacity": n_services, "starts": [(0, n_services, 0)]},
                    topics={"log_capacity": 1}, listings={"payloads": tb.listing_payloads}, schedule=schedule)
