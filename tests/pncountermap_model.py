"""TEST INFRASTRUCTURE ONLY.  A plain model of the reference's PNCounterMap = ORMap[A, PNCounter] on
top of tests/crdt_model.ORSet, and a BSP restatement of a PNCounterMap-only engine run.

    DD = akka-distributed-data/src/main/scala/akka/cluster/ddata

  PNCounterMap.increment / decrement   DD/PNCounterMap.scala:105-106,139-141
  ORMap.updated / remove / merge       DD/ORMap.scala:308-334,361-366,379-409 (dryMerge)
  PNCounter.change / merge             DD/PNCounter.scala:173-178,180-183

Arbitrary-precision ints throughout: a slot past 2^64 - 1 raises SlotRange (the engine reports
AGX_ERANGE), and `to_words` refuses what the layout cannot hold.
"""
from __future__ import annotations

import numpy as np

from akka_amd.engine import CRDT_WORDS, Kind, Op
from tests import crdt_model as M
from tests.crdt_cases import crdt_peer
from tests.lwwmap_model import WIDE, LwwModel

NODES, ELEMS = M.NODES, M.ELEMS
PNCMAP_WORDS = CRDT_WORDS[Kind.PNCOUNTERMAP]
assert PNCMAP_WORDS == 1296
CTR_WORD, SLOTS = 272, 16
U64_MAX = (1 << 64) - 1
COUNT_MAX = (1 << 18) - 1
ZERO = (0,) * SLOTS


class SlotRange(Exception):
    """A slot would pass 2^64 - 1 (the reference's BigInt would not wrap; AGX_ERANGE)."""


def counter_value(slots: tuple) -> int:
    """PNCounter.value (DD/PNCounter.scala:73): increments less decrements."""
    return sum(slots[:NODES]) - sum(slots[NODES:])


def counter_change(slots: tuple, node: int, n: int) -> tuple:
    """PNCounter.change (DD/PNCounter.scala:173-178): n > 0 raises the node's increments slot, n < 0 its
    decrements slot, n = 0 leaves the counter as it is."""
    if n == 0:
        return slots
    i = node if n > 0 else NODES + node
    out = list(slots)
    out[i] += abs(n)
    if out[i] > U64_MAX:
        raise SlotRange((i, out[i]))
    return tuple(out)


def counter_merge(a: tuple, b: tuple) -> tuple:
    """PNCounter.merge (DD/PNCounter.scala:180-183): GCounter.merge of both halves, the slot-wise maximum."""
    return tuple(max(x, y) for x, y in zip(a, b))


class PNCounterMap:
    """PNCounterMap.underlying = ORMap(keys: ORSet, values: {key: PNCounter}); a counter is 16 ints
    (increments of node 0..7, then decrements of node 0..7)."""

    def __init__(self, keys=None, values=None):
        self.keys = keys.copy() if keys is not None else M.ORSet()
        self.values = dict(values or {})

    def copy(self) -> "PNCounterMap":
        return PNCounterMap(self.keys, self.values)

    def __eq__(self, other):
        return self.keys == other.keys and self.values == other.values

    def __repr__(self):
        return f"PNCounterMap({self.keys}, {({k: counter_value(v) for k, v in self.values.items()})})"

    @property
    def entries(self) -> dict:
        """PNCounterMap.entries (DD/PNCounterMap.scala:57-58)."""
        return {k: counter_value(v) for k, v in sorted(self.values.items())}

    def change(self, node: int, key: int, n: int) -> "PNCounterMap":
        """increment (n >= 0) / decrement (n <= 0): ORMap.updated(node, key, PNCounter())(_.change(node, n))
        (DD/ORMap.scala:308-334): the present counter or a fresh one, keys.add(node, key)."""
        out = PNCounterMap(self.keys.add(node, key), self.values)
        out.values[key] = counter_change(self.values.get(key, ZERO), node, n)
        return out

    def remove(self, key: int) -> "PNCounterMap":
        """ORMap.remove (DD/ORMap.scala:361-366): keys.remove, values - key."""
        out = PNCounterMap(self.keys.remove(key), self.values)
        out.values.pop(key, None)
        return out

    def merge(self, that: "PNCounterMap", census: dict | None = None) -> "PNCounterMap":
        """ORMap.merge / dryMerge (DD/ORMap.scala:379-409) over the merged keys.  `census` counts the
        both-sides merges that changed a slot of this side."""
        mk = self.keys.merge(that.keys)
        mv = {}
        for key in mk.elements:
            a, b = self.values.get(key), that.values.get(key)
            if a is not None and b is not None:
                mv[key] = counter_merge(a, b)
                if census is not None and mv[key] != a:
                    census["both_sides_changed"] = census.get("both_sides_changed", 0) + 1
            elif a is not None:
                mv[key] = a
            elif b is not None:
                mv[key] = b
            else:
                raise AssertionError(f"missing value for {key}")
        return PNCounterMap(mk, mv)

    def canonical(self) -> bool:
        """Exactly the live keys have a counter."""
        return set(self.keys.elements) == set(self.values)


def merge_all(maps) -> PNCounterMap:
    out = maps[0].copy()
    for m in maps[1:]:
        out = out.merge(m)
    return out


def to_words(m: PNCounterMap) -> np.ndarray:
    assert m.canonical(), m
    w = np.zeros(PNCMAP_WORDS, np.uint64)
    w[:M.ORSET_WORDS] = M.orset_to_words(m.keys)
    for k, slots in m.values.items():
        assert len(slots) == SLOTS and all(0 <= x <= U64_MAX for x in slots), (k, slots)
        w[CTR_WORD + SLOTS * k:CTR_WORD + SLOTS * (k + 1)] = np.array(slots, np.uint64)
    return w


def from_words(w) -> PNCounterMap:
    w = np.ascontiguousarray(np.asarray(w, np.uint64)[:PNCMAP_WORDS])
    keys = M.orset_from_words(w)
    assert not w[M.ORSET_WORDS:CTR_WORD].any(), "padding words 260..271 are not zero"
    values = {}
    for k in range(ELEMS):
        slots = tuple(int(x) for x in w[CTR_WORD + SLOTS * k:CTR_WORD + SLOTS * (k + 1)])
        if k in keys.elements:
            values[k] = slots
        else:
            assert slots == ZERO, f"key {k}: slots without a live dot {slots}"
    return PNCounterMap(keys, values)


# ------------------------------------------------------------------ the engine run
class PncModel(LwwModel):
    """A PNCounterMap-only engine, one rank: LwwModel's superstep (inbox order, bounded mailbox, throughput,
    backlog, counters, the queued / tail-dropped census) with PNCounterMap replicas and ops.  Census of its own:
    `recreated` (a count created a key that the same replica had removed earlier) and `merge_census`."""

    def __init__(self, n_actors: int, throughput: int = 5, capacity: int = 0, n_words: int = PNCMAP_WORDS,
                 max_emit: int = 1, **_layout):
        assert n_words >= PNCMAP_WORDS
        super().__init__(n_actors, throughput, capacity, max(n_words, 356), max_emit)
        self.maps = [PNCounterMap() for _ in range(self.n)]
        self.removed = [set() for _ in range(self.n)]
        self.recreated = 0
        self.merge_census = {}

    def register_range(self, first, count, kind, init_state=None):
        assert kind in (Kind.PNCOUNTERMAP, Kind.NONE)
        for i in range(count):
            self.alive[first + i] = 1 if kind == Kind.PNCOUNTERMAP else 0
            self.maps[first + i] = from_words(np.asarray(init_state, np.uint64).reshape(count, -1)[i]) \
                if init_state is not None else PNCounterMap()

    def set_lwwmap(self, *_):
        raise AssertionError("a PNCounterMap engine has no clock")

    def read_state(self):
        w = np.zeros((self.n, self.W), np.uint64)
        for a in range(self.n):
            w[a, :PNCMAP_WORDS] = to_words(self.maps[a])
        return w, self.alive.copy()

    def _apply(self, a: int, src, pay, now: int, out: list) -> bool:
        """One message; False = Behaviors.unhandled."""
        node = a % NODES
        if src == WIDE:  # a state gossip: pay is the sender's map
            self.maps[a] = self.maps[a].merge(pay, self.merge_census)
            return True
        op, arg = pay >> 24, pay & 0xFFFFFF
        if op in (Op.INCREMENT, Op.DECREMENT):
            key, n = arg & 63, arg >> 6
            if key in self.removed[a] and key not in self.maps[a].values:
                self.recreated += 1
            try:
                self.maps[a] = self.maps[a].change(node, key, n if op == Op.INCREMENT else -n)
            except SlotRange:
                self.range_error = True
            return True
        if op == Op.REMOVE and arg < ELEMS:
            if arg in self.maps[a].values:
                self.removed[a].add(arg)
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


# ------------------------------------------------------------------ tests/golden/pncountermap_kats.json
def run_kat(case, target) -> list:
    """One KAT script through `target` (a GpuEngine or a PncModel over case["replicas"] actors, nothing
    registered yet): one run per op on the one engine, every `expect` checked against the decoded state.
    Returns the state words after every op, for a comparison between two targets."""
    n = case["replicas"]
    target.register_range(0, n, Kind.PNCOUNTERMAP)
    target.set_gossip(1, 1)  # (with two replicas the peer is always the other one)
    trace = []
    for i, st in enumerate(case["script"]):
        where = f"{case['name']} step {i} {st}"
        if "expect" in st:
            words, _ = target.read_state()
            m = from_words(words[st["expect"]])
            assert m.entries == {int(k): v for k, v in st["entries"].items()}, (where, m.entries)
            continue
        if "inc" in st:
            r, key, by = st["inc"]
            target.tell([r], [Op.increment_key(key, by)])
        elif "dec" in st:
            r, key, by = st["dec"]
            target.tell([r], [Op.decrement_key(key, by)])
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
        trace.append(target.read_state()[0][:, :PNCMAP_WORDS].copy())
    return trace
