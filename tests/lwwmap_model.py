"""TEST INFRASTRUCTURE ONLY.  A plain model of the reference's LWWMap = ORMap[A, LWWRegister[B]] on
top of tests/crdt_model.ORSet, and a BSP restatement of an LWWMap-only engine run.

    DD = akka-distributed-data/src/main/scala/akka/cluster/ddata

  LWWMap.put / remove / merge       DD/LWWMap.scala:144-150,175-187
  ORMap.put / remove / merge        DD/ORMap.scala:254-265,361-366,379-409 (dryMerge)
  LWWRegister clocks                DD/LWWRegister.scala:24-38
  LWWRegister.withValue / merge     DD/LWWRegister.scala:192-199

Arbitrary-precision ints and signed timestamps throughout: a timestamp past the int64 range raises
TimestampRange (the engine reports AGX_ERANGE), and `to_words` refuses what the layout cannot hold.
"""
from __future__ import annotations

import numpy as np

from akka_amd.engine import Kind, Op
from tests import crdt_model as M
from tests.crdt_cases import crdt_peer

NODES, ELEMS = M.NODES, M.ELEMS
LWWMAP_WORDS = 356
TS_WORD, REG_U32 = 260, 648
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
VALUE_MAX = (1 << 18) - 1
WIDE = 0x80000000


class TimestampRange(Exception):
    """A timestamp would pass the int64 range (the reference's Long would wrap; AGX_ERANGE)."""


def default_clock(now: int, ts: int) -> int:
    """LWWRegister.defaultClock (DD/LWWRegister.scala:26-29), System.currentTimeMillis() = now."""
    return max(now, ts + 1)


def reverse_clock(now: int, ts: int) -> int:
    """LWWRegister.reverseClock (DD/LWWRegister.scala:37-40): first write wins."""
    return min(-now, ts - 1)


CLOCKS = {"default": default_clock, "reverse": reverse_clock}


def register_merge(this: tuple, that: tuple) -> tuple:
    """LWWRegister.merge (DD/LWWRegister.scala:194-198) on (node, value, timestamp)."""
    if that[2] > this[2]:
        return that
    if that[2] < this[2]:
        return this
    if that[0] < this[0]:
        return that
    return this


class LWWMap:
    """LWWMap.underlying = ORMap(keys: ORSet, values: {key: LWWRegister}); a register is (node, value, timestamp)."""

    def __init__(self, keys=None, values=None):
        self.keys = keys.copy() if keys is not None else M.ORSet()
        self.values = dict(values or {})

    def copy(self) -> "LWWMap":
        return LWWMap(self.keys, self.values)

    def __eq__(self, other):
        return self.keys == other.keys and self.values == other.values

    def __repr__(self):
        return f"LWWMap({self.keys}, {self.values})"

    @property
    def entries(self) -> dict:
        """LWWMap.entries (DD/LWWMap.scala:77-80)."""
        return {k: r[1] for k, r in sorted(self.values.items())}

    def put(self, node: int, key: int, value, clock, now: int) -> "LWWMap":
        """LWWMap.put (DD/LWWMap.scala:144-150): withValue on the present register (clock(timestamp)), a
        fresh LWWRegister otherwise (clock(0), DD/LWWRegister.scala:57-58); ORMap.put (DD/ORMap.scala:254-265):
        keys.add(node, key), values.updated."""
        r = self.values.get(key)
        ts = clock(now, r[2] if r is not None else 0)
        if not INT64_MIN <= ts <= INT64_MAX:
            raise TimestampRange(ts)
        out = LWWMap(self.keys.add(node, key), self.values)
        out.values[key] = (node, value, ts)
        return out

    def remove(self, key: int) -> "LWWMap":
        """ORMap.remove (DD/ORMap.scala:361-366): keys.remove, values - key."""
        out = LWWMap(self.keys.remove(key), self.values)
        out.values.pop(key, None)
        return out

    def merge(self, that: "LWWMap") -> "LWWMap":
        """ORMap.merge / dryMerge (DD/ORMap.scala:379-409) over the merged keys."""
        mk = self.keys.merge(that.keys)
        mv = {}
        for key in mk.elements:
            a, b = self.values.get(key), that.values.get(key)
            if a is not None and b is not None:
                mv[key] = register_merge(a, b)
            elif a is not None:
                mv[key] = a
            elif b is not None:
                mv[key] = b
            else:
                raise AssertionError(f"missing value for {key}")
        return LWWMap(mk, mv)

    def canonical(self) -> bool:
        """Exactly the live keys have a register."""
        return set(self.keys.elements) == set(self.values)


def merge_all(maps) -> LWWMap:
    out = maps[0].copy()
    for m in maps[1:]:
        out = out.merge(m)
    return out


def to_words(m: LWWMap) -> np.ndarray:
    assert m.canonical(), m
    w = np.zeros(LWWMAP_WORDS, np.uint64)
    w[:M.ORSET_WORDS] = M.orset_to_words(m.keys)
    u = w.view(np.uint32)
    for k, (node, value, ts) in m.values.items():
        assert 0 <= node < NODES and 0 <= value <= VALUE_MAX and INT64_MIN <= ts <= INT64_MAX, (k, node, value, ts)
        w[TS_WORD + k] = ts & ((1 << 64) - 1)
        u[REG_U32 + k] = (node << 24) | value
    return w


def from_words(w) -> LWWMap:
    w = np.ascontiguousarray(np.asarray(w, np.uint64)[:LWWMAP_WORDS])
    u = w.view(np.uint32)
    keys = M.orset_from_words(w)
    values = {}
    for k in range(ELEMS):
        t = int(w[TS_WORD + k])
        t = t - (1 << 64) if t >> 63 else t
        r = int(u[REG_U32 + k])
        if k in keys.elements:
            values[k] = (r >> 24, r & 0xFFFFFF, t)
        else:
            assert t == 0 and r == 0, f"key {k}: register without a live dot ({r:#x}, {t})"
    return LWWMap(keys, values)


# ------------------------------------------------------------------ the engine run
class LwwModel:
    """An LWWMap-only engine, one rank: the calls of GpuEngine that Workload.apply_to makes.

    superstep, per actor with mail --
      inbox = backlog ++ arrivals in (sender, emission index) order ++ staged tells;
      bounded mailbox: position p is admitted iff C == 0 or p < C, the rest are dead letters;
      drain the first min(len, max(T, 1)), T clamped to C; the backlog is the rest.
    A state gossip carries the sender's map as it was when the tick was drained.  The LWWRegister clock's
    `now` is base + s, s = the number of supersteps with mail so far, this one included."""

    def __init__(self, n_actors: int, throughput: int = 5, capacity: int = 0, n_words: int = LWWMAP_WORDS,
                 max_emit: int = 1, **_layout):
        assert n_words >= LWWMAP_WORDS
        self.n, self.W = int(n_actors), int(n_words)
        self.T, self.C, self.kmax = max(int(throughput), 1), int(capacity), int(max_emit)
        self.alive = np.zeros(self.n, np.uint8)
        self.maps = [LWWMap() for _ in range(self.n)]
        self.f, self.seed = 0, 0
        self.clock, self.base = default_clock, 0
        self.backlog, self.emitted_q, self.staged_q = [], [], []
        self.c = dict(delivered=0, dead_letters=0, unhandled=0, emitted=0, staged=0, supersteps=0, in_flight=0)
        self.queued_gossips = 0   # census: state gossips that stayed queued past a drain (rows copied forward)
        self.tail_dropped_gossips = 0
        self.inbox_sizes = []     # per superstep: messages per destination actor (bucket load checks)
        self.range_error = False

    def register_range(self, first, count, kind, init_state=None):
        assert kind in (Kind.LWWMAP, Kind.NONE)
        for i in range(count):
            self.alive[first + i] = 1 if kind == Kind.LWWMAP else 0
            self.maps[first + i] = from_words(np.asarray(init_state, np.uint64).reshape(count, -1)[i]) \
                if init_state is not None else LWWMap()

    def set_gossip(self, fanout, seed):
        self.f, self.seed = int(fanout), int(seed)

    def set_lwwmap(self, clock="default", base=0):
        self.clock, self.base = CLOCKS[clock], int(base)

    def tell(self, dst, payload, src=None):
        dst = np.atleast_1d(np.asarray(dst, dtype=np.uint32))
        pay = np.broadcast_to(np.asarray(payload, dtype=np.uint32), dst.shape)
        for d, p in zip(dst.tolist(), pay.tolist()):
            self.c["staged"] += 1
            if d >= self.n:
                self.c["dead_letters"] += 1
                continue
            self.staged_q.append((d, 0xFFFFFFFF, p))

    def read_state(self):
        w = np.zeros((self.n, self.W), np.uint64)
        for a in range(self.n):
            w[a, :LWWMAP_WORDS] = to_words(self.maps[a])
        return w, self.alive.copy()

    def close(self):
        pass

    def _apply(self, a: int, src, pay, now: int, out: list) -> bool:
        """One message; False = Behaviors.unhandled."""
        node = a % NODES
        if src == WIDE:  # a state gossip: pay is the sender's map
            self.maps[a] = self.maps[a].merge(pay)
            return True
        op, arg = pay >> 24, pay & 0xFFFFFF
        if op == Op.PUT:
            try:
                self.maps[a] = self.maps[a].put(node, arg & 63, arg >> 6, self.clock, now)
            except TimestampRange:
                self.range_error = True
            return True
        if op == Op.REMOVE and arg < ELEMS:
            self.maps[a] = self.maps[a].remove(arg)
            return True
        if op == Op.GOSSIP:
            f = self.f if self.n > 1 else 0
            if f:
                snap = self.maps[a].copy()
                for j in range(f):
                    out.append((crdt_peer(self.seed, a, arg, j, self.n), WIDE, snap))
            if arg > 0:
                out.append((a, a, Op.make(Op.GOSSIP, arg - 1)))
            return True
        return False

    def step(self) -> bool:
        msgs = self.backlog + self.emitted_q + self.staged_q
        if not msgs:
            return False
        now = self.base + self.c["supersteps"] + 1
        inbox = {}
        for d, s, p in msgs:
            inbox.setdefault(d, []).append((s, p))
        self.backlog, out = [], []
        sizes = np.zeros(self.n, np.int64)
        for a, q in inbox.items():
            sizes[a] = len(q)
        self.inbox_sizes.append(sizes)
        for a in sorted(inbox):
            q = inbox[a]
            L = len(q)
            if not self.alive[a]:
                self.c["dead_letters"] += L
                continue
            C, T = self.C, (min(self.T, self.C) if self.C else self.T)
            keep = L if C == 0 else min(L, C)
            self.c["dead_letters"] += L - keep
            self.tail_dropped_gossips += sum(1 for s, _ in q[keep:] if s == WIDE)
            nd = min(keep, T)
            n0 = len(out)
            for s, p in q[:nd]:
                self.c["delivered"] += 1
                if not self._apply(a, s, p, now, out):
                    self.c["unhandled"] += 1
            self.c["emitted"] += len(out) - n0
            self.queued_gossips += sum(1 for s, _ in q[nd:keep] if s == WIDE)
            self.backlog += [(a, s, p) for s, p in q[nd:keep]]
        self.emitted_q, self.staged_q = out, []
        self.c["supersteps"] += 1
        return True

    def run(self, max_supersteps: int = 1 << 30) -> dict:
        i = 0
        while i < max_supersteps and self.step():
            i += 1
        self.c["in_flight"] = len(self.backlog) + len(self.emitted_q) + len(self.staged_q)
        return dict(self.c)

    def max_bucket_inbox(self, bucket_actors: int) -> int:
        """The largest inbox (backlog included) any bucket of `bucket_actors` actors saw so far."""
        best = 0
        for s in self.inbox_sizes:
            pad = (-s.size) % bucket_actors
            best = max(best, int(np.pad(s, (0, pad)).reshape(-1, bucket_actors).sum(axis=1).max()))
        return best

    def converged(self) -> bool:
        live = [self.maps[a] for a in range(self.n) if self.alive[a]]
        return all(m == live[0] for m in live[1:])


# ------------------------------------------------------------------ tests/golden/lwwmap_kats.json
def kat_initial_words(case) -> np.ndarray:
    """The `init` steps of a KAT case as (replicas, 356) state words: replica r as if node r % 8 had put the
    listed (key, value, timestamp) in order, or a copy of another replica's init."""
    maps = [LWWMap() for _ in range(case["replicas"])]
    for st in case["script"]:
        if "init" in st:
            r = st["init"]
            if "of" in st:
                maps[r] = maps[st["of"]].copy()
            else:
                for key, value, ts in st["puts"]:
                    maps[r] = maps[r].put(r % NODES, key, value, lambda now, cur, ts=ts: ts, 0)
    return np.stack([to_words(m) for m in maps])


def run_kat(case, target) -> list:
    """One KAT script through `target` (a GpuEngine or an LwwModel over case["replicas"] actors, nothing
    registered yet): one run per op on the one engine, every `expect` checked against the decoded state.
    Returns the state words after every op, for a comparison between two targets."""
    n = case["replicas"]
    target.register_range(0, n, Kind.LWWMAP, kat_initial_words(case))
    target.set_gossip(1, 1)  # (with two replicas the peer is always the other one)
    target.set_lwwmap(case.get("clock", "default"), case.get("base", 0))
    trace = []
    for i, st in enumerate(case["script"]):
        where = f"{case['name']} step {i} {st}"
        if "init" in st:
            continue
        if "expect" in st or "expect_ts" in st:
            words, _ = target.read_state()
            m = from_words(words[st.get("expect", st.get("expect_ts"))])
            if "expect" in st:
                assert m.entries == {int(k): v for k, v in st["entries"].items()}, (where, m.entries)
            else:
                assert m.values[st["key"]][2] == st["ts"], (where, m.values[st["key"]])
            continue
        if "put" in st:
            r, key, value = st["put"]
            target.tell([r], [Op.put(key, value)])
        elif "puts" in st:
            r, key, values = st["puts"]
            target.tell([r] * len(values), [Op.put(key, v) for v in values])
        elif "remove" in st:
            r, key = st["remove"]
            target.tell([r], [Op.make(Op.REMOVE, key)])
        elif "gossip" in st:
            s, r = st["gossip"]
            assert n == 2 and {s, r} == {0, 1}, where
            target.tell([s], [Op.make(Op.GOSSIP, 0)])
        else:
            raise AssertionError(where)
        stats = target.run()
        stats = stats if isinstance(stats, dict) else {k: getattr(stats, k) for k in ("unhandled", "in_flight", "dead_letters")}
        assert stats["unhandled"] == 0 and stats["in_flight"] == 0 and stats["dead_letters"] == 0, (where, stats)
        trace.append(target.read_state()[0][:, :LWWMAP_WORDS].copy())
    return trace
