"""TEST INFRASTRUCTURE ONLY.  A plain model of the reference's ORMultiMap = ORMap[A, ORSet[B]] (the plain
ORMultiMap.empty, withValueDeltas = false) on top of tests/crdt_model.ORSet -- the key set and every value set
are that ORSet, with Python ints --, and a BSP restatement of an ORMultiMap-only engine run.

    DD = akka-distributed-data/src/main/scala/akka/cluster/ddata

  ORMultiMap.merge / put / remove                DD/ORMultiMap.scala:78-91,182-189,216-225
  addBinding / removeBinding / replaceBinding    DD/ORMultiMap.scala:248-252,277-290,310-318
  ORMap.updated / remove / merge                 DD/ORMap.scala:308-334,361-366,379-409 (dryMerge)
  ORSet.add / remove / clear / merge             DD/ORSet.scala:339,380,404,427-

Nothing wraps: a version past 2^32 - 1 raises VersionRange (the engine reports AGX_ERANGE), and `to_words`
refuses what the layout cannot hold.
"""
from __future__ import annotations

import numpy as np

from akka_amd.engine import CRDT_WORDS, Kind, Op
from tests import crdt_model as M
from tests.crdt_cases import crdt_peer
from tests.lwwmap_model import WIDE, LwwModel

NODES, ELEMS, VALUES = M.NODES, M.ELEMS, 8
ORMM_WORDS = CRDT_WORDS[Kind.ORMULTIMAP]
assert ORMM_WORDS == 2576
SET_WORD, SET_U32 = 272, 72
U32_MAX = (1 << 32) - 1


class VersionRange(Exception):
    """A key-set or value-set version would pass 2^32 - 1 (the reference's Long would not wrap; AGX_ERANGE)."""


class ORMultiMap:
    """ORMultiMap.underlying = ORMap(keys: ORSet, values: {key: ORSet of value indices})."""

    def __init__(self, keys=None, values=None):
        self.keys = keys.copy() if keys is not None else M.ORSet()
        self.values = {k: s.copy() for k, s in (values or {}).items()}

    def copy(self) -> "ORMultiMap":
        return ORMultiMap(self.keys, self.values)

    def __eq__(self, other):
        return self.keys == other.keys and self.values == other.values

    def __repr__(self):
        return f"ORMultiMap({self.keys}, {self.values})"

    # ---- reads (DD/ORMultiMap.scala:96-135)
    @property
    def entries(self) -> dict:
        return {k: frozenset(s.elements) for k, s in sorted(self.values.items())}

    def get(self, key: int):
        s = self.values.get(key)
        return None if s is None else frozenset(s.elements)

    def get_or_else(self, key: int, default):
        s = self.get(key)
        return default if s is None else s

    def contains(self, key: int) -> bool:
        return key in self.keys.elements

    @property
    def size(self) -> int:
        return len(self.keys.elements)

    # ---- writes
    def _updated(self, node: int, key: int, modify) -> "ORMultiMap":
        """ORMap.updated(node, key, ORSet.empty)(modify) (DD/ORMap.scala:308-334): the present set or an empty
        one, keys.add(node, key) always."""
        out = ORMultiMap(self.keys.add(node, key), self.values)
        out.values[key] = modify(self.values.get(key, M.ORSet()))
        return out

    def _remove_key(self, key: int) -> "ORMultiMap":
        """ORMap.remove (DD/ORMap.scala:361-366): keys.remove, values - key."""
        out = ORMultiMap(self.keys.remove(key), self.values)
        out.values.pop(key, None)
        return out

    def add_binding(self, node: int, key: int, value: int) -> "ORMultiMap":
        """DD/ORMultiMap.scala:248-252."""
        return self._updated(node, key, lambda s: s.add(node, value))

    def remove_binding(self, node: int, key: int, value: int) -> "ORMultiMap":
        """DD/ORMultiMap.scala:277-290: a set left empty is followed by ORMap.remove(node, key)."""
        u = self._updated(node, key, lambda s: s.remove(value))
        return u._remove_key(key) if not u.values[key].elements else u

    def put(self, node: int, key: int, values) -> "ORMultiMap":
        """DD/ORMultiMap.scala:182-189: clear(), then add of every value -- in ascending value index (the
        reference folds over a Scala Set in its iteration order; pinned here by construction)."""
        def modify(s):
            s = s.clear()
            for v in sorted(set(values)):
                s = s.add(node, v)
            return s
        return self._updated(node, key, modify)

    def replace_binding(self, node: int, key: int, old: int, new: int) -> "ORMultiMap":
        """DD/ORMultiMap.scala:310-318: `this` when old == new."""
        if old == new:
            return self
        return self.add_binding(node, key, new).remove_binding(node, key, old)

    def remove(self, node: int, key: int) -> "ORMultiMap":
        """DD/ORMultiMap.scala:216-225 (withValueDeltas = false): ORMap.remove."""
        return self._remove_key(key)

    def merge(self, that: "ORMultiMap", census: dict | None = None) -> "ORMultiMap":
        """ORMap.merge / dryMerge (DD/ORMap.scala:379-409) over the merged keys.  `census` counts the both-sides
        merges that changed this side's set."""
        mk = self.keys.merge(that.keys)
        mv = {}
        for key in mk.elements:
            a, b = self.values.get(key), that.values.get(key)
            if a is not None and b is not None:
                mv[key] = a.merge(b)
                if census is not None and mv[key] != a:
                    census["both_sides_changed"] = census.get("both_sides_changed", 0) + 1
            elif a is not None:
                mv[key] = a
            elif b is not None:
                mv[key] = b
            else:
                raise AssertionError(f"missing value for {key}")
        return ORMultiMap(mk, mv)

    def canonical(self) -> bool:
        """Exactly the live keys have a value set."""
        return set(self.keys.elements) == set(self.values)

    def max_version(self) -> int:
        vs = list(self.keys.vvector.values())
        for s in self.values.values():
            vs += list(s.vvector.values())
        return max(vs, default=0)


def merge_all(maps) -> ORMultiMap:
    out = maps[0].copy()
    for m in maps[1:]:
        out = out.merge(m)
    return out


def to_words(m: ORMultiMap) -> np.ndarray:
    assert m.canonical(), m
    w = np.zeros(ORMM_WORDS, np.uint64)
    w[:M.ORSET_WORDS] = M.orset_to_words(m.keys)
    u = w.view(np.uint32)
    for k, s in m.values.items():
        base = 2 * SET_WORD + SET_U32 * k
        for n, v in s.vvector.items():
            assert 0 <= n < NODES and 0 < v <= U32_MAX, (k, n, v)
            u[base + n] = v
        for val, dot in s.elements.items():
            assert 0 <= val < VALUES and dot, (k, val, dot)
            for n, v in dot.items():
                assert 0 <= n < NODES and 0 < v <= U32_MAX, (k, val, n, v)
                u[base + NODES * (1 + val) + n] = v
    return w


def from_words(w) -> ORMultiMap:
    w = np.ascontiguousarray(np.asarray(w, np.uint64)[:ORMM_WORDS])
    keys = M.orset_from_words(w)
    assert not w[M.ORSET_WORDS:SET_WORD].any(), "padding words 260..271 are not zero"
    u = w.view(np.uint32)
    values = {}
    for k in range(ELEMS):
        b = u[2 * SET_WORD + SET_U32 * k:2 * SET_WORD + SET_U32 * (k + 1)]
        if k in keys.elements:
            vv = {n: int(b[n]) for n in range(NODES) if b[n]}
            el = {}
            for val in range(VALUES):
                dot = {n: int(b[NODES * (1 + val) + n]) for n in range(NODES) if b[NODES * (1 + val) + n]}
                if dot:
                    el[val] = dot
            values[k] = M.ORSet(el, vv)
        else:
            assert not b.any(), f"key {k}: a value set without a live key dot"
    return ORMultiMap(keys, values)


def row_u32(m: ORMultiMap) -> int:
    """The used length of m's snapshot row: header, the live key dots rounded up to 4, 72 u32 per live key."""
    dots = sum(len(d) for d in m.keys.elements.values())
    return 32 + (dots + 3) // 4 * 4 + SET_U32 * len(m.values)


def apply_op(m: ORMultiMap, node: int, pay: int):
    """One control tell on the data type; None = Behaviors.unhandled (an unknown op or an argument out of range)."""
    op, arg = pay >> 24, pay & 0xFFFFFF
    key, a, b = arg & 63, (arg >> 6) & 7, (arg >> 9) & 7
    if op == Op.ADD and arg < 512:
        out = m.add_binding(node, key, a)
    elif op == Op.REMOVE_BINDING and arg < 512:
        out = m.remove_binding(node, key, a)
    elif op == Op.PUT and arg < 64 * 256:
        out = m.put(node, key, [v for v in range(VALUES) if (arg >> 6) >> v & 1])
    elif op == Op.REPLACE_BINDING and arg < 4096:
        out = m.replace_binding(node, key, a, b)
    elif op == Op.REMOVE and arg < ELEMS:
        out = m.remove(node, arg)
    else:
        return None
    if out.max_version() > U32_MAX:
        raise VersionRange(out.max_version())
    return out


# ------------------------------------------------------------------ the engine run
class MmModel(LwwModel):
    """An ORMultiMap-only engine, one rank: LwwModel's superstep (inbox order, bounded mailbox, throughput,
    backlog, counters, the queued / tail-dropped census) with ORMultiMap replicas and ops -- the same superstep as
    PncModel.  Census of its own: `rebound` (a binding created a key that the same replica had dropped earlier),
    `key_removals` (ops that dropped a live key) and `merge_census`."""

    def __init__(self, n_actors: int, throughput: int = 5, capacity: int = 0, n_words: int = ORMM_WORDS,
                 max_emit: int = 1, **_layout):
        assert n_words >= ORMM_WORDS
        super().__init__(n_actors, throughput, capacity, n_words, max_emit)
        self.maps = [ORMultiMap() for _ in range(self.n)]
        self.removed = [set() for _ in range(self.n)]
        self.rebound = 0
        self.key_removals = 0
        self.merge_census = {}

    def register_range(self, first, count, kind, init_state=None):
        assert kind in (Kind.ORMULTIMAP, Kind.NONE)
        for i in range(count):
            self.alive[first + i] = 1 if kind == Kind.ORMULTIMAP else 0
            self.maps[first + i] = from_words(np.asarray(init_state, np.uint64).reshape(count, -1)[i]) \
                if init_state is not None else ORMultiMap()

    def set_lwwmap(self, *_):
        raise AssertionError("an ORMultiMap engine has no clock")

    def read_state(self):
        w = np.zeros((self.n, self.W), np.uint64)
        for a in range(self.n):
            w[a, :ORMM_WORDS] = to_words(self.maps[a])
        return w, self.alive.copy()

    def _apply(self, a: int, src, pay, now: int, out: list) -> bool:
        """One message; False = Behaviors.unhandled."""
        node = a % NODES
        if src == WIDE:  # a state gossip: pay is the sender's map
            self.maps[a] = self.maps[a].merge(pay, self.merge_census)
            return True
        op, arg = pay >> 24, pay & 0xFFFFFF
        if op == Op.GOSSIP:
            f = self.f if self.n > 1 else 0
            if f:
                snap = self.maps[a].copy()
                for j in range(f):
                    out.append((crdt_peer(self.seed, a, arg, j, self.n), WIDE, snap))
            if arg > 0:
                out.append((a, a, Op.make(Op.GOSSIP, arg - 1)))
            return True
        before = self.maps[a]
        try:
            after = apply_op(before, node, pay)
        except VersionRange:
            self.range_error = True
            return True
        if after is None:
            return False
        key = arg & 63
        if key in before.values and key not in after.values:
            self.removed[a].add(key)
            self.key_removals += 1
        if key in self.removed[a] and key not in before.values and key in after.values:
            self.rebound += 1
        self.maps[a] = after
        return True


# ------------------------------------------------------------------ tests/golden/ormultimap_kats.json
def kat_op(case, st) -> int:
    """The control tell of one script step: strings map to key and value indices in the fixture."""
    K, V = case["keys"], case["values"]
    if "add" in st:
        _, k, v = st["add"]
        return Op.add_binding(K[k], V[v])
    if "unbind" in st:
        _, k, v = st["unbind"]
        return Op.remove_binding(K[k], V[v])
    if "put" in st:
        _, k, vs = st["put"]
        return Op.put_set(K[k], [V[v] for v in vs])
    if "replace" in st:
        _, k, o, n = st["replace"]
        return Op.replace_binding(K[k], V[o], V[n])
    if "remove" in st:
        _, k = st["remove"]
        return Op.make(Op.REMOVE, K[k])
    raise AssertionError(st)


def kat_initial_words(case) -> np.ndarray:
    """`init`: {replica: [[node, step], ...]} -- a replica's state as the spec builds it with the data type, where
    one map takes ops by more than one node (a replica of the engine is one node)."""
    w = np.zeros((case["replicas"], ORMM_WORDS), np.uint64)
    for r, ops in case.get("init", {}).items():
        m = ORMultiMap()
        for node, st in ops:
            m = apply_op(m, node, kat_op(case, st))
        w[int(r)] = to_words(m)
    return w


def run_kat(case, target) -> list:
    """One KAT script through `target` (a GpuEngine or an MmModel over case["replicas"] actors, nothing registered
    yet): one run per op on the one engine, every `expect` checked against the decoded state.  Returns the state
    words after every op, for a comparison between two targets."""
    n = case["replicas"]
    K, V = case["keys"], case["values"]
    target.register_range(0, n, Kind.ORMULTIMAP, kat_initial_words(case) if "init" in case else None)
    target.set_gossip(1, 1)  # (with two replicas the peer is always the other one)
    trace = []
    for i, st in enumerate(case["script"]):
        where = f"{case['name']} step {i} {st}"
        if "expect" in st:
            words, _ = target.read_state()
            m = from_words(words[st["expect"]])
            if "entries" in st:
                want = {K[k]: frozenset(V[v] for v in vs) for k, vs in st["entries"].items()}
                assert m.entries == want, (where, m.entries)
            for k, present in st.get("contains", {}).items():
                assert m.contains(K[k]) == present, (where, k)
            for k, vs in st.get("get_or_else", {}).items():
                assert m.get_or_else(K[k], frozenset(V[v] for v in vs["default"])) == frozenset(V[v] for v in vs["is"]), (where, k)
            continue
        if "gossip" in st:
            s, r = st["gossip"]
            assert n == 2 and {s, r} == {0, 1}, where
            target.tell([s], [Op.make(Op.GOSSIP, 0)])
        else:
            target.tell([next(iter(st.values()))[0]], [kat_op(case, st)])
        stats = target.run()
        stats = stats if isinstance(stats, dict) else {k: getattr(stats, k) for k in ("unhandled", "in_flight", "dead_letters")}
        assert stats["unhandled"] == 0 and stats["in_flight"] == 0 and stats["dead_letters"] == 0, (where, stats)
        trace.append(target.read_state()[0][:, :ORMM_WORDS].copy())
    return trace
