"""A pure Python model of an engine with router logics: ReceptionistModel plus DESIGN.md §2.12
(consistent-hashing and random routing), in plain Python.

  * `murmur_string_hash` restates MurmurHash.stringHash (akka-actor routing/MurmurHash.scala:115-129, with extendHash
    :80-81, nextMagicA / nextMagicB :84-87 and finalizeHash :90-97) and `concatenate_node_hash`
    ConsistentHash.concatenateNodeHash (routing/ConsistentHash.scala:134-139), both in Java Int arithmetic: wrapping
    32-bit products and sums, `>>>` for the shifts;
  * `ConsistentHashRing` restates ConsistentHash.apply (:119-128) and nodeFor (:76-83,100-110): a node is an actor id
    as a decimal string, its points are concatenate_node_hash(murmur_string_hash(str(id)), 1..factor), the ring is
    ordered by (hash as a signed i32, id), nodeFor(h) is the first entry with hash >= h, else entry 0.  On equal
    hashes the smaller id wins (the reference's SortedMap keeps one of them, by Set iteration order);
  * the ring of a hashed key in force during tick t holds the points of the actors whose bit was set at the end of
    tick t - 1 (the listing's timing; the listing's capacity does not cut the ring);
  * a random route draws listing[fanout_rand(seed, self, (c & 0xFFFFFF) | 0x02000000, 0) mod size], c the low 32 bits
    of the counter word, which grows by one on a hit only.

Not fast; not meant to be."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, UNHANDLED, fanout_rand
from tests.receptionist_model import NONE, ReceptionistModel

ROUTER_INFO_KEYS = ("hashed", "random", "ring_rebuilds")
RANDOM_TAG = 0x02000000


def _i32(x: int) -> int:
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def _rotl(x: int, r: int) -> int:
    x &= M32
    return ((x << r) | (x >> (32 - r))) & M32


def extend_hash(h: int, value: int, magic_a: int, magic_b: int) -> int:
    """MurmurHash.scala:80-81: (hash ^ rotl(value * magicA, 11) * magicB) * 3 + visibleMixer"""
    return (((h ^ ((_rotl(value * magic_a, 11) * magic_b) & M32)) * 3) + 0x52dce729) & M32


def finalize_hash(h: int) -> int:
    """MurmurHash.scala:90-97"""
    i = (h ^ (h >> 16)) & M32
    i = (i * 0x85ebca6b) & M32
    i ^= i >> 13
    i = (i * 0xc2b2ae35) & M32
    i ^= i >> 16
    return i


def murmur_string_hash(s: str) -> int:
    """MurmurHash.scala:115-129, as the unsigned pattern of the Int it returns."""
    h = ((len(s) * 0xf7ca7fd2) & M32) ^ 0x971e137b  # startHash(s.length * seedString)
    c, k = 0x95543787, 0x2ad7eb25                    # hiddenMagicA, hiddenMagicB
    j = 0
    while j + 1 < len(s):
        i = ((ord(s[j]) << 16) + ord(s[j + 1])) & M32
        h = extend_hash(h, i, c, k)
        c = (c * 5 + 0x7b7d159c) & M32               # nextMagicA
        k = (k * 5 + 0x6bce6396) & M32               # nextMagicB
        j += 2
    if j < len(s):
        h = extend_hash(h, ord(s[j]), c, k)
    return finalize_hash(h)


def concatenate_node_hash(node_hash: int, vnode: int) -> int:
    """ConsistentHash.scala:134-139"""
    return finalize_hash(extend_hash((node_hash ^ 0x971e137b) & M32, vnode, 0x95543787, 0x2ad7eb25))


class ConsistentHashRing:
    """ConsistentHash(ids.map(_.toString), factor) (ConsistentHash.scala:119-128) with nodeFor (:76-83,100-110)."""

    def __init__(self, ids, factor: int):
        if factor < 1:
            raise ValueError("virtualNodesFactor must be >= 1")  # (ConsistentHash.scala:26)
        self.factor = factor
        self.entries = sorted((_i32(concatenate_node_hash(murmur_string_hash(str(a)), v)), int(a))
                              for a in ids for v in range(1, factor + 1))
        self._hashes = [h for h, _ in self.entries]

    @classmethod
    def from_entries(cls, entries):
        """A ring of given (signed hash, id) entries (tests of the ordering and collision rules)."""
        r = cls((), 1)
        r.entries = sorted((int(h), int(a)) for h, a in entries)
        r._hashes = [h for h, _ in r.entries]
        return r

    def __len__(self):
        return len(self.entries)

    def node_for_hash(self, h_signed: int):
        if not self.entries:
            raise LookupError("Can't get node for [%d] from an empty node ring" % h_signed)  # (IllegalStateException)
        j = bisect_left(self._hashes, h_signed)
        return self.entries[0 if j == len(self.entries) else j][1]

    def node_for(self, key: str):
        if not self.entries:
            raise LookupError("Can't get node for [%s] from an empty node ring" % key)
        return self.node_for_hash(_i32(murmur_string_hash(key)))

    def hashes_u32(self) -> np.ndarray:
        return np.asarray([h & M32 for h, _ in self.entries], np.uint32)

    def ids(self) -> np.ndarray:
        return np.asarray([a for _, a in self.entries], np.uint32)


def random_index(seed: int, self_id: int, counter: int, size: int) -> int:
    """The index a random route draws; fanout_rand's domain tag 0x02000000 is this logic's own."""
    return fanout_rand(seed, self_id, (counter & 0xFFFFFF) | RANDOM_TAG, 0) % size


class RouterModel(ReceptionistModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.logics = False
        self.hashed_mask = 0
        self.vnf = 0
        self.rseed = 0
        self.rings = [ConsistentHashRing((), 1) for _ in range(8)]
        self.rinfo = dict.fromkeys(ROUTER_INFO_KEYS, 0)

    # ------------------------------------------------------------ the engine's calls
    def set_router_logics(self, hashed_keys_mask, virtual_nodes_factor=0, seed=0):
        assert self.n_keys and not self.logics and not hashed_keys_mask >> self.n_keys
        assert not hashed_keys_mask or 1 <= virtual_nodes_factor <= 64
        self.logics, self.hashed_mask, self.rseed = True, int(hashed_keys_mask), int(seed)
        self.vnf = int(virtual_nodes_factor) if hashed_keys_mask else 0
        for k in range(8):  # (what is registered already is in the first rings: no ring_rebuilds for it)
            if (self.hashed_mask >> k) & 1:
                self.rings[k] = ConsistentHashRing(np.flatnonzero((self.mask >> k) & 1).tolist(), self.vnf)

    def _rebuild(self, keys):
        keys = list(keys)
        super()._rebuild(keys)
        for k in keys:
            if (self.hashed_mask >> k) & 1:
                # (the ring holds the points of every member: the listing's capacity cuts the listing alone)
                self.rings[k] = ConsistentHashRing(np.flatnonzero((self.mask >> k) & 1).tolist(), self.vnf)
                self.rinfo["ring_rebuilds"] += 1

    def router_info(self):
        d = dict(self.rinfo)
        d["ring_size"] = [len(self.rings[k]) if (self.hashed_mask >> k) & 1 else 0 for k in range(8)]
        return d

    def read_hash_ring(self, key):
        assert (self.hashed_mask >> key) & 1
        return self.rings[key].hashes_u32(), self.rings[key].ids()

    # ------------------------------------------------------------ behaviours
    def _compiled(self, a, w, src, pay):
        """ReceptionistModel._compiled with ROUTE_HASHED and ROUTE_RANDOM."""
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is None or b >= t.n_behaviors:
            return UNHANDLED
        for ci in range(int(t.first[b]), int(t.first[b + 1])):
            C = t.cases[ci]
            if not self._cmp(C.cmp1, self._operand(C.src1, C.word1, C.k1, pay, w, src, a),
                             self._operand(C.src2, C.word2, C.k2, pay, w, src, a)):
                continue
            if not self._cmp(C.cmp2, self._operand(C.src3, C.word3, C.k3, pay, w, src, a),
                             self._operand(C.src4, C.word4, C.k4, pay, w, src, a)):
                continue
            for i in range(C.act_first, C.act_first + C.act_count):
                A = t.acts[i]
                v = self._operand(A.src, A.sword, A.k, pay, w, src, a)
                msg = ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32)
                x, bit = A.word & 1, 1 << (A.pad1 & 7)
                if A.op == typed.A_SET:
                    w[x] = v
                elif A.op == typed.A_ADD:
                    w[x] = (w[x] + v) & M64
                elif A.op == typed.A_MAX:
                    w[x] = max(w[x], v)
                elif A.op == typed.A_MIN:
                    w[x] = min(w[x], v)
                elif A.op == typed.A_REGISTER:
                    if not int(self.mask[a]) & bit:
                        self.mask[a] |= bit
                        self.info["registered"] += 1
                elif A.op == typed.A_DEREGISTER:
                    if int(self.mask[a]) & bit:
                        self.mask[a] &= ~bit & 0xFF
                        self.info["deregistered"] += 1
                elif A.op in (typed.A_TELL, typed.A_ROUTE):
                    d = 0
                    if A.op == typed.A_TELL or A.pad0 & (typed.ROUTE_BY_INDEX | typed.ROUTE_HASHED):
                        if A.dsrc == typed.V_SELF and A.op == typed.A_TELL:
                            d = (a + A.dk) % self.n
                        else:
                            d = self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a)
                    ref = min(d, M32)
                    if A.op == typed.A_ROUTE:
                        key = A.pad1 & 7
                        L = self.listing[key]
                        if A.pad0 & typed.ROUTE_HASHED:
                            assert self.logics and (self.hashed_mask >> key) & 1
                            ring = self.rings[key]
                            ref = ring.node_for(str(d & M32)) if len(ring) else NONE  # (the low 32 bits of x)
                            if ref != NONE:
                                self.rinfo["hashed"] += 1
                        elif A.pad0 & typed.ROUTE_RANDOM:
                            assert self.logics
                            if L:  # (no routee: the counter stays)
                                ref = L[random_index(self.rseed, a, w[x] & M32, len(L))]
                                w[x] = (w[x] + 1) & M64
                                self.rinfo["random"] += 1
                            else:
                                ref = NONE
                        elif not L:
                            ref = NONE
                        elif A.pad0 & typed.ROUTE_BY_INDEX:
                            ref = L[d % len(L)]
                        else:
                            j = bisect_left(L, w[x])
                            ref = L[0 if j == len(L) else j]
                            w[x] = ref + 1
                        self.info["no_routees" if ref == NONE else "routed"] += 1
                    self._emit(src if A.pad0 & typed.ROUTE_KEEP_SENDER else a, ref, msg)
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED
