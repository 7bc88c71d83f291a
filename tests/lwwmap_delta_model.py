"""TEST INFRASTRUCTURE ONLY.  A plain model of delta replication for LWWMap = ORMap[A, LWWRegister[B]], written
from the Scala text with immutable values and a sequential dryMergeDelta, on tests/crdt_model.ORSet and
tests/lwwmap_model.LWWMap; and a BSP restatement of an LWWMap engine in agx_set_lwwmap_delta mode.

    DD = akka-distributed-data/src/main/scala/akka/cluster/ddata

  ORSet.AddDeltaOp / RemoveDeltaOp / FullStateDeltaOp / DeltaGroup   DD/ORSet.scala:43-116
  ORSet.add / remove / clear (the deltas they record)                DD/ORSet.scala:339-351,380-387,404-412
  ORSet.dryMerge / mergeDelta / mergeRemoveDelta                     DD/ORSet.scala:434-501
  ORMap.AtomicDeltaOp / PutDeltaOp / RemoveDeltaOp / DeltaGroup      DD/ORMap.scala:56-164
  ORMap.put / remove                                                 DD/ORMap.scala:254-265,361-366
  ORMap.dryMergeDelta / mergeDelta                                   DD/ORMap.scala:425-503
  LWWMap.put / remove / mergeDelta                                   DD/LWWMap.scala:144-150,175-187,199-200
  DeltaPropagationSelector                                           DD/DeltaPropagationSelector.scala:44-57,95-155
  Replicator delta bookkeeping, tick, receiveDeltaPropagation        DD/Replicator.scala:910-917,1646-1695,1953-2027
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from akka_amd.engine import DELTA_WRITE, Kind, Op
from tests import crdt_model as M
from tests import lwwmap_model as L
from tests.crdt_cases import crdt_key_peer
from tests.prio_model import fanout_rand

NODES, ELEMS = M.NODES, M.ELEMS
LWWMAP_WORDS = L.LWWMAP_WORDS
DELTA_WORDS = 880          # AGX_LWWMAP_DELTA_WORDS
ENV_U32 = 2 * LWWMAP_WORDS  # u32 index of deltaVersions
RING_U32 = ENV_U32 + 24
ENT_U32 = 16
DELTA_LOG = 64
WIDE = L.WIDE
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ ORSet deltas
@dataclass(frozen=True)
class AddDeltaOp:
    underlying: M.ORSet


@dataclass(frozen=True)
class RemoveDeltaOp:
    underlying: M.ORSet

    def __post_init__(self):  # (DD/ORSet.scala:79-80)
        assert len(self.underlying.elements) == 1, "RemoveDeltaOp should contain one removed element"


@dataclass(frozen=True)
class FullStateDeltaOp:
    underlying: M.ORSet


@dataclass(frozen=True)
class SetDeltaGroup:
    ops: tuple


def set_delta_merge(this, that):
    """ORSet.DeltaOp.merge (DD/ORSet.scala:59-66,82-85,90-93,102-111)."""
    if isinstance(this, SetDeltaGroup):
        if isinstance(that, AddDeltaOp):  # merge AddDeltaOp into last AddDeltaOp in the group, if possible
            last = this.ops[-1]
            if isinstance(last, AddDeltaOp):
                return SetDeltaGroup(this.ops[:-1] + (set_delta_merge(last, that),))
            return SetDeltaGroup(this.ops + (that,))
        if isinstance(that, SetDeltaGroup):
            return SetDeltaGroup(this.ops + that.ops)
        return SetDeltaGroup(this.ops + (that,))
    if isinstance(this, AddDeltaOp) and isinstance(that, AddDeltaOp):
        u, t = this.underlying, that.underlying
        # concatElementsMap (:68-74): that's entries replace this's
        return AddDeltaOp(M.ORSet({**u.elements, **t.elements}, M.vv_merge(u.vvector, t.vvector)))
    if isinstance(that, SetDeltaGroup):
        return SetDeltaGroup((this,) + that.ops)
    return SetDeltaGroup((this, that))


def set_delta_size(d) -> int:
    return len(d.ops) if isinstance(d, SetDeltaGroup) else 1


def orset_add(s: M.ORSet, node: int, element, version: int | None = None):
    """ORSet.add with the AddDeltaOp it records on a set whose delta was reset (DD/ORSet.scala:339-351).
    `version`: the new version when it comes from a clock of the caller's (a KAT's global counter)."""
    vv = dict(s.vvector)
    vv[node] = version if version is not None else vv.get(node, 0) + 1
    dot = {node: vv[node]}
    out = M.ORSet({**s.elements, element: dot}, vv)
    return out, AddDeltaOp(M.ORSet({element: dot}, dot))


def orset_remove(s: M.ORSet, node: int, element):
    """ORSet.remove with its RemoveDeltaOp (DD/ORSet.scala:380-387): the delta's set holds the element with
    deltaDot = (node -> vvector.versionAt(node)) and the remover's whole vvector."""
    v = M.vv_version_at(s.vvector, node)
    delta_dot = {node: v} if v else {}
    rm = RemoveDeltaOp(M.ORSet({element: delta_dot}, s.vvector))
    return s.remove(element), rm


def orset_clear(s: M.ORSet):
    """ORSet.clear with its FullStateDeltaOp (DD/ORSet.scala:404-412)."""
    full = M.ORSet({}, s.vvector)
    return full, FullStateDeltaOp(full)


def _raw_elements(s: M.ORSet, extra: dict) -> M.ORSet:
    """An ORSet whose elementsMap may hold an empty dot (a RemoveDeltaOp's deltaDot of a node at version 0)."""
    out = M.ORSet({}, s.vvector)
    out.elements = {e: dict(d) for e, d in extra.items()}
    return out


def orset_dry_merge(this: M.ORSet, that: M.ORSet, add_delta_op: bool) -> M.ORSet:
    """ORSet.dryMerge (DD/ORSet.scala:434-453)."""
    common = [k for k in this.elements if k in that.elements]
    entries00 = M.merge_common_keys(common, this, that)
    if add_delta_op:
        entries0 = {**entries00, **{e: d for e, d in this.elements.items() if e not in that.elements}}
    else:
        this_unique = [k for k in this.elements if k not in that.elements]
        entries0 = M.merge_disjoint_keys(this_unique, this.elements, that.vvector, entries00)
    that_unique = [k for k in that.elements if k not in this.elements]
    entries = M.merge_disjoint_keys(that_unique, that.elements, this.vvector, entries0)
    return M.ORSet(entries, M.vv_merge(this.vvector, that.vvector))


def orset_merge_remove_delta(this: M.ORSet, op: RemoveDeltaOp) -> M.ORSet:
    """ORSet.mergeRemoveDelta (DD/ORSet.scala:471-501)."""
    that = op.underlying
    (elem, that_dot), = that.elements.items()
    delete_dots = list(that.vvector.items())
    delete_nodes = [n for n, _ in delete_dots]
    this_dot = this.elements.get(elem)
    greater = all(this_dot is not None and M.vv_version_at(this_dot, n) <= v for n, v in delete_dots)
    elements = dict(this.elements)
    if greater and this_dot is not None and all(n in delete_nodes for n in this_dot):
        del elements[elem]
    return M.ORSet(elements, M.vv_merge(this.vvector, that_dot))


def orset_merge_delta(this: M.ORSet, d) -> M.ORSet:
    """ORSet.mergeDelta (DD/ORSet.scala:455-469)."""
    if isinstance(d, AddDeltaOp):
        return orset_dry_merge(this, d.underlying, True)
    if isinstance(d, RemoveDeltaOp):
        return orset_merge_remove_delta(this, d)
    if isinstance(d, FullStateDeltaOp):
        return orset_dry_merge(this, d.underlying, False)
    acc = this
    for op in d.ops:
        assert not isinstance(op, SetDeltaGroup), "ORSet.DeltaGroup should not be nested"
        acc = orset_merge_delta(acc, op)
    return acc


# ------------------------------------------------------------------ ORMap delta ops (of an LWWMap)
@dataclass(frozen=True)
class PutDeltaOp:
    underlying: object   # the ORSet.DeltaOp of the key (an AddDeltaOp)
    key: int
    value: tuple         # the full LWWRegister (node, value, timestamp)


@dataclass(frozen=True)
class MapRemoveDeltaOp:
    underlying: object   # an ORSet RemoveDeltaOp


@dataclass(frozen=True)
class DeltaGroup:
    ops: tuple


class _NoDelta:
    def __repr__(self):
        return "NoDeltaPlaceholder"


NO_DELTA = _NoDelta()  # Replicator.Internal.DeltaPropagation.NoDeltaPlaceholder (merge = this)


def _atomic_merge(this, that):
    """AtomicDeltaOp.merge / PutDeltaOp.merge (DD/ORMap.scala:62-65,76-91; no UpdateDeltaOp in an LWWMap)."""
    if isinstance(this, PutDeltaOp) and isinstance(that, PutDeltaOp) and this.key == that.key:
        return PutDeltaOp(set_delta_merge(this.underlying, that.underlying), that.key, that.value)
    if isinstance(that, DeltaGroup):
        return DeltaGroup((this,) + that.ops)
    return DeltaGroup((this, that))


def delta_merge(this, that):
    """ORMap.DeltaOp.merge, DeltaGroup.merge included (DD/ORMap.scala:140-158)."""
    if not isinstance(this, DeltaGroup):
        return _atomic_merge(this, that)
    if isinstance(that, DeltaGroup):
        return DeltaGroup(this.ops + that.ops)
    last = this.ops[-1]
    if isinstance(last, PutDeltaOp):
        merged = _atomic_merge(last, that)
        if isinstance(merged, DeltaGroup):
            return DeltaGroup(this.ops[:-1] + merged.ops)
        return DeltaGroup(this.ops[:-1] + (merged,))
    return DeltaGroup(this.ops + (that,))


def delta_size(d) -> int:
    return len(d.ops) if isinstance(d, DeltaGroup) else 1


def delta_ops(d) -> tuple:
    return d.ops if isinstance(d, DeltaGroup) else (d,)


def put_delta(m: L.LWWMap, node: int, key: int, value, clock, now: int):
    """LWWMap.put -> ORMap.put (DD/LWWMap.scala:144-150, DD/ORMap.scala:254-265): keys.resetDelta.add, and
    PutDeltaOp(newKeys.delta.get, key -> the full register)."""
    r = m.values.get(key)
    ts = clock(now, r[2] if r is not None else 0)
    if not L.INT64_MIN <= ts <= L.INT64_MAX:
        raise L.TimestampRange(ts)
    keys, add = orset_add(m.keys, node, key)
    reg = (node, value, ts)
    return L.LWWMap(keys, {**m.values, key: reg}), PutDeltaOp(add, key, reg)


def remove_delta(m: L.LWWMap, node: int, key: int):
    """ORMap.remove (DD/ORMap.scala:361-366): keys.resetDelta.remove, values - key, RemoveDeltaOp(newKeys.delta.get)."""
    keys, rm = orset_remove(m.keys, node, key)
    return L.LWWMap(keys, {k: v for k, v in m.values.items() if k != key}), MapRemoveDeltaOp(rm)


def dry_merge_delta(this: L.LWWMap, delta) -> L.LWWMap:
    """ORMap.dryMergeDelta (DD/ORMap.scala:425-498), withValueDeltas = false: the ops in order over a copy."""
    merged_keys = this.keys
    merged_values = {k: v for k, v in this.values.items() if k in this.keys.elements}
    for op in delta_ops(delta):
        if isinstance(op, PutDeltaOp):
            merged_keys = orset_merge_delta(merged_keys, op.underlying)
            merged_values = {**merged_values, op.key: op.value}  # put is destructive
        elif isinstance(op, MapRemoveDeltaOp):
            assert isinstance(op.underlying, RemoveDeltaOp), "ORMap.RemoveDeltaOp must contain ORSet.RemoveDeltaOp inside"
            removed = next(iter(op.underlying.underlying.elements))
            merged_values = {k: v for k, v in merged_values.items() if k != removed}
            merged_keys = orset_merge_delta(merged_keys, op.underlying)
        else:
            raise AssertionError("Cannot nest DeltaGroups")
    out = L.LWWMap(merged_keys)
    out.values = merged_values  # (may hold a value whose key is not live: this.merge below decides)
    return out


def merge_delta(this: L.LWWMap, delta) -> L.LWWMap:
    """ORMap.mergeDelta (DD/ORMap.scala:500-503): this.merge(dryMergeDelta(thatDelta))."""
    return this.merge(dry_merge_delta(this, delta))


def collect_group(entries: list, max_delta_size: int):
    """DeltaPropagationSelector.collectPropagations' reduceLeft (DD/DeltaPropagationSelector.scala:111-126)."""
    group = entries[0]
    for d2 in entries[1:]:
        if d2 is NO_DELTA or group is NO_DELTA:
            merged = NO_DELTA
        else:
            merged = delta_merge(group, d2)
        if merged is not NO_DELTA and delta_size(merged) >= max_delta_size:
            merged = NO_DELTA  # discard too large deltas
        group = merged
    return group


# ------------------------------------------------------------------ selector helpers
def key_size(a: int, n: int) -> int:
    return min(NODES, n - (a & ~(NODES - 1)))


def slice_size(na: int) -> int:
    """DeltaPropagationSelector.nodesSliceSize (gossipIntervalDivisor 5): max(2, min(na / 5 + 1, 10)), at most na."""
    return min(max(na // 5 + 1, 2), min(na, 10))


def slice_node(node: int, na: int, s: int, rr: int, i: int) -> int:
    k = i if na <= s else (rr % na + i) % na
    return k + 1 if k >= node else k


def writer_op(seed: int, a: int, k: int) -> int:
    """The writer client's seeded update of DELTA_TICK countdown k (include/akka_gpu.h "LWWMap delta replication")."""
    r = fanout_rand(seed, a, k | 0x04000000, 0)
    key = (r >> 48) & 7
    if (r >> 40) & 3:
        return Op.put(key, (r >> 8) & L.VALUE_MAX)
    return Op.make(Op.REMOVE, key)


# ------------------------------------------------------------------ the engine run
class LwwDeltaModel(L.LwwModel):
    """An LWWMap engine after set_lwwmap_delta: LwwModel's superstep with the Replicator's delta bookkeeping per
    replica -- deltaVersions, deltaCounter, round robin, deltaSentToNode, the deltaEntries (and their image in
    the 64-entry ring).  A DeltaPropagation carries (from node, fromSeqNr, toSeqNr, group); a full-state gossip
    the sender's map and deltaVersions.  Census counters say what a run exercised."""

    def __init__(self, n_actors: int, throughput: int = 5, capacity: int = 0, n_words: int = DELTA_WORDS,
                 max_emit: int = 4, **_layout):
        super().__init__(n_actors, throughput, capacity, max(n_words, LWWMAP_WORDS), max_emit)
        assert n_words >= DELTA_WORDS
        n = self.n
        self.max_delta = 0
        self.dv = [[0] * NODES for _ in range(n)]
        self.ctr = [0] * n
        self.rr = [0] * n
        self.sent = [[0] * NODES for _ in range(n)]
        self.entries = [dict() for _ in range(n)]            # seqNr -> delta op
        self.ring = np.zeros((n, DELTA_LOG, ENT_U32), np.uint32)
        self.capacity_error = False
        self.census = dict(coalesced_puts=0, uncoalesced_groups=0, placeholders=0, skipped_props=0, stale_props=0,
                           queued_props=0, dropped_props=0, applied_props=0, groups=0, single_seq_groups=0)

    def register_range(self, first, count, kind, init_state=None):
        if init_state is not None:
            init_state = np.asarray(init_state, np.uint64).reshape(count, -1)
            assert not init_state[:, LWWMAP_WORDS:].any(), "the model seeds data words only"
        super().register_range(first, count, kind, init_state)

    def set_lwwmap_delta(self, max_delta_size=50):
        assert 1 <= max_delta_size <= 50 and self.kmax >= 4
        self.max_delta = int(max_delta_size)

    def read_state(self):
        w, alive = super().read_state()
        u = w.view(np.uint32)
        for a in range(self.n):
            u[a, ENV_U32:ENV_U32 + 8] = self.dv[a]
            u[a, ENV_U32 + 8] = self.ctr[a]
            u[a, ENV_U32 + 9] = self.rr[a] & M32
            u[a, ENV_U32 + 10:ENV_U32 + 18] = self.sent[a]
            u[a, RING_U32:RING_U32 + DELTA_LOG * ENT_U32] = self.ring[a].reshape(-1)
        return w, alive

    def _record(self, a: int, op):
        """DeltaPropagationSelector.update: the next seqNr's entry (and its ring image)."""
        node, m = a % NODES, key_size(a, self.n)
        self.ctr[a] += 1
        q = self.ctr[a]
        if q > DELTA_LOG and any(x != node and self.sent[a][x] < q - DELTA_LOG for x in range(m)):
            self.capacity_error = True
        self.entries[a][q] = op
        e = np.zeros(ENT_U32, np.uint32)
        e[0] = q
        if isinstance(op, PutDeltaOp):
            (key, dot), = op.underlying.underlying.elements.items()
            rnode, value, ts = op.value
            e[1] = 1 | (key << 8)
            e[2] = dot[node]
            e[3] = (rnode << 24) | value
            e[4], e[5] = ts & M32, (ts >> 32) & M32
        else:
            s = op.underlying.underlying
            (key, _), = s.elements.items()
            e[1] = 2 | (key << 8)
            for x, v in s.vvector.items():
                e[8 + x] = v
        self.ring[a, q % DELTA_LOG] = e
        lo = min([self.sent[a][x] for x in range(m) if x != node], default=q)
        for old in [s for s in self.entries[a] if s <= min(lo, q - DELTA_LOG)]:  # (cleanupDeltaEntries: sent everywhere)
            del self.entries[a][old]

    def _tick(self, a: int, arg: int, out: list):
        k = arg & 0xFFFF
        node = a % NODES
        if arg & DELTA_WRITE:
            out.append((a, a, writer_op(self.seed, a, k)))
        na = key_size(a, self.n) - 1
        if na:
            sz = slice_size(na)
            for i in range(min(na, sz)):
                x = slice_node(node, na, sz, self.rr[a], i)
                j = self.sent[a][x]
                if self.ctr[a] <= j:
                    continue
                ents = [self.entries[a][q] for q in range(j + 1, self.ctr[a] + 1)]
                group = collect_group(ents, self.max_delta)
                self.sent[a][x] = self.ctr[a]
                self.census["groups"] += 1
                if group is NO_DELTA:
                    self.census["placeholders"] += 1
                    continue
                self.census["single_seq_groups"] += len(ents) == 1
                self.census["coalesced_puts"] += len(ents) - delta_size(group)
                self.census["uncoalesced_groups"] += 1 if delta_size(group) >= 2 else 0
                out.append((a - node + x, WIDE, ("delta", node, j + 1, self.ctr[a], group)))
            self.rr[a] += sz
        if k > 0:
            out.append((a, a, Op.make(Op.DELTA_TICK, (k - 1) | (arg & DELTA_WRITE))))

    def _apply(self, a: int, src, pay, now: int, out: list) -> bool:
        node = a % NODES
        if src == WIDE:
            if pay[0] == "delta":  # receiveDeltaPropagation (DD/Replicator.scala:1965-2027): causal delivery
                _, frm, lo, hi, group = pay
                cur = self.dv[a][frm]
                if cur >= hi:
                    self.census["stale_props"] += 1
                elif lo > cur + 1:
                    self.census["skipped_props"] += 1
                else:
                    self.maps[a] = merge_delta(self.maps[a], group)
                    assert self.maps[a].canonical()
                    self.dv[a][frm] = hi
                    self.census["applied_props"] += 1
                return True
            _, that, dv = pay  # DataEnvelope.merge
            self.maps[a] = self.maps[a].merge(that)
            self.dv[a] = [max(x, y) for x, y in zip(self.dv[a], dv)]
            return True
        op, arg = pay >> 24, pay & 0xFFFFFF
        if op == Op.PUT:
            try:
                self.maps[a], d = put_delta(self.maps[a], node, arg & 63, arg >> 6, self.clock, now)
                self._record(a, d)
            except L.TimestampRange:
                self.range_error = True
            return True
        if op == Op.REMOVE and arg < ELEMS:
            self.maps[a], d = remove_delta(self.maps[a], node, arg)
            self._record(a, d)
            return True
        if op == Op.GOSSIP:
            f = self.f if self.n > 1 and key_size(a, self.n) > 1 else 0
            if f:
                snap = ("full", self.maps[a].copy(), tuple(self.dv[a]))
                for j in range(f):
                    out.append((crdt_key_peer(self.seed, a, arg, j, self.n), WIDE, snap))
            if arg > 0:
                out.append((a, a, Op.make(Op.GOSSIP, arg - 1)))
            return True
        if op == Op.DELTA_TICK:
            self._tick(a, arg, out)
            return True
        return False

    def step(self) -> bool:
        """LwwModel.step, with the census of queued and dropped DeltaPropagations."""
        msgs = self.backlog + self.emitted_q + self.staged_q
        inbox = {}
        for d, s, p in msgs:
            inbox.setdefault(d, []).append((s, p))
        for a, q in inbox.items():
            if not self.alive[a]:
                continue
            C, T = self.C, (min(self.T, self.C) if self.C else self.T)
            keep = len(q) if C == 0 else min(len(q), C)
            isprop = lambda sp: sp[0] == WIDE and sp[1][0] == "delta"
            self.census["dropped_props"] += sum(1 for sp in q[keep:] if isprop(sp))
            self.census["queued_props"] += sum(1 for sp in q[min(keep, T):keep] if isprop(sp))
        return super().step()

    def key_converged(self) -> bool:
        """Every key's replicas hold one value."""
        for g in range(0, self.n, NODES):
            ms = [self.maps[a] for a in range(g, min(g + NODES, self.n)) if self.alive[a]]
            if any(m != ms[0] for m in ms[1:]):
                return False
        return True


# ------------------------------------------------------------------ tests/golden/lwwmap_delta_kats.json
def run_script(case) -> dict:
    """A KAT op script on the plain functions.  Names bind maps and deltas:
      ["put", out, in, node, key, value]   out = in.put (timestamps: the script's own counter), delta "<out>.d"
      ["remove", out, in, node, key]       out = in.remove, delta "<out>.d"
      ["merge", out, a, b]                 out = a.merge(b)
      ["merge_delta", out, a, delta]       out = a.mergeDelta(delta)
      ["dmerge", out, d1, d2]              out = d1.merge(d2)   (ORMap.DeltaOp.merge)
    """
    vals, now = {"empty": L.LWWMap()}, [0]
    for op in case["ops"]:
        k = op[0]
        if k == "put":
            now[0] += 1
            vals[op[1]], vals[op[1] + ".d"] = put_delta(vals[op[2]], op[3], op[4], op[5], L.default_clock, now[0])
        elif k == "remove":
            vals[op[1]], vals[op[1] + ".d"] = remove_delta(vals[op[2]], op[3], op[4])
        elif k == "merge":
            vals[op[1]] = vals[op[2]].merge(vals[op[3]])
        elif k == "merge_delta":
            vals[op[1]] = merge_delta(vals[op[2]], vals[op[3]])
        elif k == "dmerge":
            vals[op[1]] = delta_merge(vals[op[2]], vals[op[3]])
        else:
            raise AssertionError(op)
        if isinstance(vals[op[1]], L.LWWMap):
            assert vals[op[1]].canonical(), (case["name"], op)
    return vals


def check_script(case, vals):
    for chk in case["checks"]:
        k = chk[0]
        if k == "entries":
            assert vals[chk[1]].entries == {int(a): b for a, b in chk[2].items()}, (case["name"], chk, vals[chk[1]].entries)
        elif k == "equal":
            assert vals[chk[1]] == vals[chk[2]], (case["name"], chk)
        elif k == "ops":  # deltaSize and the op types of a delta
            d = vals[chk[1]]
            assert delta_size(d) == chk[2], (case["name"], chk, d)
            kinds = ["put" if isinstance(o, PutDeltaOp) else "remove" for o in delta_ops(d)]
            assert kinds == chk[3], (case["name"], chk, kinds)
        elif k == "last_put":  # the group's last op: a put of this key, this value, this dot version
            o = delta_ops(vals[chk[1]])[-1]
            (key, dot), = o.underlying.underlying.elements.items()
            assert isinstance(o, PutDeltaOp) and (o.key, o.value[1]) == (chk[2], chk[3]) and key == chk[2], (case["name"], chk, o)
            assert list(dot.values()) == [chk[4]] and list(o.underlying.underlying.vvector.values()) == [chk[4]], (case["name"], chk, o)
        else:
            raise AssertionError(chk)
