"""TEST INFRASTRUCTURE ONLY.  A plain arbitrary-precision model of the reference's ORSet,
VersionVector, GCounter and PNCounter, written from the Scala sources as they are structured
(maps of node -> version, common / disjoint keys), not from the engine's per-entry formula:

    DD = akka-distributed-data/src/main/scala/akka/cluster/ddata

A VersionVector is a dict {node: version} of Python ints with no zero entries (a missing node is
Timestamp.Zero, DD/VersionVector.scala:76-80).  An ORSet is (elements {element: dot}, vvector) with
dot a VersionVector.  Counters are dicts {node: int}.  Nothing here wraps: a version or a counter
slot past the engine's field width shows as a value that `to_words` refuses.

`to_words` / `from_words` convert to and from the engine layout (include/akka_gpu.h "CRDT
behaviours"): ORSet u64[260] = 64 x 8 u32 dots then 8 u32 versions, little endian; GCounter u64[8];
PNCounter u64[16] = increments then decrements.
"""
from __future__ import annotations

import numpy as np

NODES = 8
ELEMS = 64
ORSET_WORDS = 260


# ------------------------------------------------------------------ VersionVector
def vv_version_at(vv: dict, node: int) -> int:
    """VersionVector.versionAt (DD/VersionVector.scala:283-287,338-341): Zero when absent."""
    return vv.get(node, 0)


def vv_compare(a: dict, b: dict) -> str:
    """VersionVector.compareTo = compareOnlyTo(FullOrder) (DD/VersionVector.scala:184-234,251-253): walk both node-sorted entry
    lists; '==' Same, '<' Before, '>' After, '<>' Concurrent.  A node present on one side only
    counts against the other side."""
    if a == b:
        return "=="
    ia, ib = sorted(a.items()), sorted(b.items())
    order = "=="
    i = j = 0

    def step(cur, new):
        return new if cur in ("==", new) else "<>"

    while i < len(ia) and j < len(ib) and order != "<>":
        (n1, v1), (n2, v2) = ia[i], ib[j]
        if n1 == n2:  # both have the node: compare the versions
            if v1 < v2:
                order = step(order, "<")
            elif v1 > v2:
                order = step(order, ">")
            i, j = i + 1, j + 1
        elif n1 < n2:  # this has a node that has none: this is After for that node
            order = step(order, ">")
            i += 1
        else:
            order = step(order, "<")
            j += 1
    if order != "<>" and i < len(ia):
        order = step(order, ">")
    if order != "<>" and j < len(ib):
        order = step(order, "<")
    return order


def vv_merge(a: dict, b: dict) -> dict:
    """VersionVector.merge (DD/VersionVector.scala:296-308 One, :355-375 Many): for every node of
    that, keep the larger version."""
    out = dict(a)
    for node, v in b.items():
        if v > out.get(node, 0):
            out[node] = v
    return out


def vv_increment(vv: dict, node: int) -> dict:
    """VersionVector.+ / increment (DD/VersionVector.scala:277-281,331-336).  The reference draws the
    version from the JVM-wide Timestamp.counter; a replica's own monotonic counter
    (versionAt(node) + 1) orders the same way per node, which is all a merge compares."""
    out = dict(vv)
    out[node] = vv.get(node, 0) + 1
    return out


# ------------------------------------------------------------------ ORSet
class ORSet:
    """DD/ORSet.scala: elementsMap {element: Dot} and vvector."""

    def __init__(self, elements=None, vvector=None):
        self.elements = {e: dict(d) for e, d in (elements or {}).items()}
        self.vvector = dict(vvector or {})

    def copy(self) -> "ORSet":
        return ORSet(self.elements, self.vvector)

    def __eq__(self, other):
        return self.elements == other.elements and self.vvector == other.vvector

    def __repr__(self):
        return f"ORSet({self.elements}, {self.vvector})"

    def element_set(self) -> set:
        return set(self.elements)

    def add(self, node: int, element) -> "ORSet":
        """ORSet.add (DD/ORSet.scala:339-351): newVvector = vvector + node; the element's dot is
        replaced by the one birth dot (node -> newVvector.versionAt(node))."""
        vv = vv_increment(self.vvector, node)
        out = ORSet(self.elements, vv)
        out.elements[element] = {node: vv[node]}
        return out

    def remove(self, element) -> "ORSet":
        """ORSet.remove (DD/ORSet.scala:380-387): elementsMap - element, vvector unchanged."""
        out = self.copy()
        out.elements.pop(element, None)
        return out

    def clear(self) -> "ORSet":
        """ORSet.clear (DD/ORSet.scala:404-412): no elements, the history (vvector) kept."""
        return ORSet({}, self.vvector)

    def merge(self, that: "ORSet") -> "ORSet":
        """ORSet.merge = dryMerge(that, addDeltaOp = false) (DD/ORSet.scala:427-453)."""
        common = [k for k in self.elements if k in that.elements]
        entries = merge_common_keys(common, self, that)
        this_unique = [k for k in self.elements if k not in that.elements]
        entries = merge_disjoint_keys(this_unique, self.elements, that.vvector, entries)
        that_unique = [k for k in that.elements if k not in self.elements]
        entries = merge_disjoint_keys(that_unique, that.elements, self.vvector, entries)
        return ORSet(entries, vv_merge(self.vvector, that.vvector))


def subtract_dots(dot: dict, vvector: dict) -> dict:
    """ORSet.subtractDots (DD/ORSet.scala:127-158): a dot entry that is <= the vvector's entry for
    its node is dominated and dropped."""
    return {node: v1 for node, v1 in dot.items() if not vv_version_at(vvector, node) >= v1}


def merge_common_keys(common, lhs: ORSet, rhs: ORSet) -> dict:
    """ORSet.mergeCommonKeys (DD/ORSet.scala:170-230).  The four (One|Many, One|Many) cases of the
    source differ in representation only: common dots (same node and version on both sides) are
    kept; of the others each side keeps what the other side's vvector has not seen; a key whose
    merged dot is empty is dropped."""
    acc = {}
    for k in common:
        l, r = lhs.elements[k], rhs.elements[k]
        if len(l) == 1 and len(r) == 1 and l == r:  # (:176-179) one single common dot
            acc[k] = dict(l)
            continue
        common_dots = {n: v for n, v in l.items() if r.get(n) == v}                      # (:190-192)
        l_unique = {n: v for n, v in l.items() if n not in common_dots}                  # (:194)
        r_unique = {n: v for n, v in r.items() if n not in common_dots}                  # (:195)
        l_keep = subtract_dots(l_unique, rhs.vvector)                                    # (:196)
        r_keep = subtract_dots(r_unique, lhs.vvector)                                    # (:197)
        merged = vv_merge(vv_merge(l_keep, r_keep), common_dots)                         # (:198)
        if merged:                                                                       # (:200-201)
            acc[k] = merged
    return acc


def merge_disjoint_keys(keys, elements: dict, vvector: dict, acc: dict) -> dict:
    """ORSet.mergeDisjointKeys (DD/ORSet.scala:243-259): a key on one side only is dropped when the
    other side's vvector is After or Same as its dot (the other side saw the add and removed it);
    otherwise it keeps the dots not yet seen."""
    acc = dict(acc)
    for k in keys:
        dots = elements[k]
        if vv_compare(vvector, dots) in (">", "=="):
            continue
        acc[k] = subtract_dots(dots, vvector)
    return acc


def merge_all(states) -> ORSet:
    """Left fold of ORSet.merge over a non-empty list."""
    out = states[0].copy()
    for s in states[1:]:
        out = out.merge(s)
    return out


def orset_to_words(s: ORSet) -> np.ndarray:
    w = np.zeros(ORSET_WORDS, np.uint64)
    u = w.view(np.uint32)
    for e, dot in s.elements.items():
        assert 0 <= e < ELEMS and dot, (e, dot)
        for n, v in dot.items():
            assert 0 <= n < NODES and 0 < v < 1 << 32, (e, n, v)
            u[e * NODES + n] = v
    for n, v in s.vvector.items():
        assert 0 <= n < NODES and 0 < v < 1 << 32, (n, v)
        u[ELEMS * NODES + n] = v
    return w


def orset_from_words(w) -> ORSet:
    u = np.ascontiguousarray(np.asarray(w, np.uint64)[:ORSET_WORDS]).view(np.uint32)
    elements = {}
    for e in range(ELEMS):
        dot = {n: int(u[e * NODES + n]) for n in range(NODES) if u[e * NODES + n]}
        if dot:
            elements[e] = dot
    vv = {n: int(u[ELEMS * NODES + n]) for n in range(NODES) if u[ELEMS * NODES + n]}
    return ORSet(elements, vv)


# ------------------------------------------------------------------ counters
def gcounter_increment(state: dict, node: int, n: int) -> dict:
    """GCounter.increment (DD/GCounter.scala:97-111): state(node) + n, unbounded (BigInt, :53)."""
    out = dict(state)
    out[node] = out.get(node, 0) + n
    return out


def gcounter_value(state: dict) -> int:
    """GCounter.value (DD/GCounter.scala:62-64): the sum of every node's count."""
    return sum(state.values())


def gcounter_merge(a: dict, b: dict) -> dict:
    """GCounter.merge (DD/GCounter.scala:113-125): per node the larger count."""
    out = dict(a)
    for node, v in b.items():
        if v > out.get(node, 0):
            out[node] = v
    return out


def pncounter_merge(a: tuple, b: tuple) -> tuple:
    """PNCounter.merge (DD/PNCounter.scala:176-179): increments and decrements merge as GCounters."""
    return gcounter_merge(a[0], b[0]), gcounter_merge(a[1], b[1])


def pncounter_value(a: tuple) -> int:
    """PNCounter.value (DD/PNCounter.scala:56-60): increments.value - decrements.value."""
    return gcounter_value(a[0]) - gcounter_value(a[1])


def gcounter_to_words(state: dict, slots: int = NODES) -> np.ndarray:
    w = np.zeros(slots, np.uint64)
    for n, v in state.items():
        assert 0 <= n < slots and 0 <= v < 1 << 64, (n, v)
        w[n] = v
    return w


def gcounter_from_words(w, slots: int = NODES) -> dict:
    return {n: int(x) for n, x in enumerate(np.asarray(w, np.uint64)[:slots]) if x}


def pncounter_to_words(a: tuple) -> np.ndarray:
    return np.concatenate([gcounter_to_words(a[0]), gcounter_to_words(a[1])])


def pncounter_from_words(w) -> tuple:
    w = np.asarray(w, np.uint64)
    return gcounter_from_words(w[:NODES]), gcounter_from_words(w[NODES:2 * NODES])
