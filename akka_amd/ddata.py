"""Read side of the replicated data types the engine holds: decode a replica's state words.

    from akka_amd.ddata import LWWMap
    words, _ = eng.read_state()
    m = LWWMap.from_words(words[replica])
    m.entries            # {key: value}
    m.get(3), m.contains(3), m.size, m.timestamp(3), m.updated_by(3)

The layout is include/akka_gpu.h "LWWMap replicas": the ORSet key set (64 keys x 8 u32 dots, 8 u32
version vector), 64 int64 timestamps, 64 u32 registers (updatedBy node << 24 | value).  Writes go
through the engine (Op.put, Op.REMOVE); `to_words` exists to seed replicas (register_range).  A row of an
engine with delta replication (set_lwwmap_delta) is wider: `from_words` decodes its first 356 words as before
and `delta_versions` reads the 8 DataEnvelope.deltaVersions behind them.

    from akka_amd.ddata import PNCounterMap
    c = PNCounterMap.from_words(words[replica])
    c.entries            # {key: signed value}
    c.get(3), c.contains(3), c.size, c.increments(3), c.decrements(3)

"PNCounterMap replicas": the same key set, 12 words of padding, then 16 u64 slots per key (8 increments, 8
decrements, one per node).  Writes: Op.increment_key, Op.decrement_key, Op.REMOVE.

    from akka_amd.ddata import ORMultiMap
    m = ORMultiMap.from_words(words[replica])
    m.entries            # {key: frozenset of value indices}
    m.get(3), m.get_or_else(3, frozenset()), m.contains(3), m.size, m.is_empty

"ORMultiMap replicas": the same key set and padding, then 72 u32 per key: the value set's own version vector
(8 u32) and 8 values x 8 node dots.  Writes: Op.add_binding, Op.remove_binding, Op.put_set, Op.replace_binding,
Op.REMOVE.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .engine import ORMM_VALUES, CRDT_NODES, CRDT_WORDS, Kind, LWW_VALUE_MAX, ORSET_ELEMS

LWWMAP_WORDS = CRDT_WORDS[Kind.LWWMAP]
_VV = ORSET_ELEMS * CRDT_NODES          # u32 index of the version vector
_TS = CRDT_WORDS[Kind.ORSET]            # u64 index of key 0's timestamp
_REG = 2 * (_TS + ORSET_ELEMS)          # u32 index of key 0's register
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
PNCMAP_WORDS = CRDT_WORDS[Kind.PNCOUNTERMAP]
_CTR = 272                              # u64 index of key 0's slots (AGX_PNCMAP_CTR_WORD)
_SLOTS = 2 * CRDT_NODES                 # u64 slots per key: increments, then decrements
ORMM_WORDS = CRDT_WORDS[Kind.ORMULTIMAP]
_SET = 2 * 272                          # u32 index of key 0's value set (AGX_ORMM_SET_WORD)
_SET_U32 = CRDT_NODES + ORMM_VALUES * CRDT_NODES  # AGX_ORMM_SET_U32: version vector, then 8 values x 8 node dots


@dataclass
class LWWMap:
    """One replica's LWWMap: per live key its dots {node: version}, and its LWWRegister
    (updatedBy node, value, timestamp); the key set's version vector {node: version}."""
    dots: dict = field(default_factory=dict)        # key -> {node: version}, live keys only
    vvector: dict = field(default_factory=dict)     # node -> version
    registers: dict = field(default_factory=dict)   # key -> (node, value, timestamp)
    # DataEnvelope.deltaVersions per node (the seqNr last applied from it) of a delta-width row, else None;
    # not part of the data: `entries` and `to_words` ignore it
    delta_versions: tuple | None = field(default=None, compare=False)

    @classmethod
    def from_words(cls, row) -> "LWWMap":
        full = np.ascontiguousarray(np.asarray(row, np.uint64))
        w = np.ascontiguousarray(full[:LWWMAP_WORDS])
        if w.size != LWWMAP_WORDS:
            raise ValueError(f"an LWWMap replica has {LWWMAP_WORDS} state words, got {w.size}")
        u = w.view(np.uint32)
        ts = w[_TS:_TS + ORSET_ELEMS].view(np.int64)
        m = cls()
        for k in range(ORSET_ELEMS):
            d = {n: int(u[k * CRDT_NODES + n]) for n in range(CRDT_NODES) if u[k * CRDT_NODES + n]}
            r = int(u[_REG + k])
            if d:
                m.dots[k] = d
                m.registers[k] = (r >> 24, r & 0xFFFFFF, int(ts[k]))
            elif r or ts[k]:
                raise ValueError(f"key {k} has no live dot but a register ({r:#x}, {int(ts[k])}): not canonical")
        m.vvector = {n: int(u[_VV + n]) for n in range(CRDT_NODES) if u[_VV + n]}
        if full.size >= LWWMAP_WORDS + CRDT_NODES // 2:  # (a delta-width row: the envelope area follows the data)
            m.delta_versions = tuple(int(x) for x in full[LWWMAP_WORDS:LWWMAP_WORDS + CRDT_NODES // 2].view(np.uint32))
        return m

    def to_words(self) -> np.ndarray:
        w = np.zeros(LWWMAP_WORDS, np.uint64)
        u = w.view(np.uint32)
        ts = w[_TS:_TS + ORSET_ELEMS].view(np.int64)
        if set(self.dots) != set(self.registers):
            raise ValueError("every live key has exactly one register")
        for k, d in self.dots.items():
            if not 0 <= k < ORSET_ELEMS or not d:
                raise ValueError(f"key {k}: outside the 64-key universe, or without a dot")
            for n, v in d.items():
                if not (0 <= n < CRDT_NODES and 0 < v < 1 << 32):
                    raise ValueError(f"dot ({k}, {n}) -> {v} does not fit the layout")
                u[k * CRDT_NODES + n] = v
            node, value, t = self.registers[k]
            if not (0 <= node < CRDT_NODES and 0 <= value <= LWW_VALUE_MAX and INT64_MIN <= t <= INT64_MAX):
                raise ValueError(f"register of key {k} {self.registers[k]} does not fit the layout")
            u[_REG + k] = (node << 24) | value
            ts[k] = t
        for n, v in self.vvector.items():
            if not (0 <= n < CRDT_NODES and 0 < v < 1 << 32):
                raise ValueError(f"version vector entry {n} -> {v} does not fit the layout")
            u[_VV + n] = v
        return w

    @property
    def entries(self) -> dict:
        """LWWMap.entries: {key: value}."""
        return {k: r[1] for k, r in sorted(self.registers.items())}

    def get(self, key: int):
        r = self.registers.get(key)
        return None if r is None else r[1]

    def contains(self, key: int) -> bool:
        return key in self.registers

    @property
    def size(self) -> int:
        return len(self.registers)

    def timestamp(self, key: int):
        r = self.registers.get(key)
        return None if r is None else r[2]

    def updated_by(self, key: int):
        r = self.registers.get(key)
        return None if r is None else r[0]


@dataclass
class PNCounterMap:
    """One replica's PNCounterMap: per live key its dots {node: version} and its PNCounter as 16 slots
    (increments of node 0..7, then decrements of node 0..7); the key set's version vector {node: version}."""
    dots: dict = field(default_factory=dict)        # key -> {node: version}, live keys only
    vvector: dict = field(default_factory=dict)     # node -> version
    slots: dict = field(default_factory=dict)       # key -> tuple of 16 ints

    @classmethod
    def from_words(cls, row) -> "PNCounterMap":
        w = np.ascontiguousarray(np.asarray(row, np.uint64)[:PNCMAP_WORDS])
        if w.size != PNCMAP_WORDS:
            raise ValueError(f"a PNCounterMap replica has {PNCMAP_WORDS} state words, got {w.size}")
        u = w.view(np.uint32)
        if w[_TS:_CTR].any():
            raise ValueError("the padding words 260..271 are not zero: not canonical")
        m = cls()
        for k in range(ORSET_ELEMS):
            d = {n: int(u[k * CRDT_NODES + n]) for n in range(CRDT_NODES) if u[k * CRDT_NODES + n]}
            sl = tuple(int(x) for x in w[_CTR + _SLOTS * k:_CTR + _SLOTS * (k + 1)])
            if d:
                m.dots[k] = d
                m.slots[k] = sl
            elif any(sl):
                raise ValueError(f"key {k} has no live dot but non-zero slots: not canonical")
        m.vvector = {n: int(u[_VV + n]) for n in range(CRDT_NODES) if u[_VV + n]}
        return m

    def to_words(self) -> np.ndarray:
        w = np.zeros(PNCMAP_WORDS, np.uint64)
        u = w.view(np.uint32)
        if set(self.dots) != set(self.slots):
            raise ValueError("every live key has exactly one counter")
        for k, d in self.dots.items():
            if not 0 <= k < ORSET_ELEMS or not d:
                raise ValueError(f"key {k}: outside the 64-key universe, or without a dot")
            for n, v in d.items():
                if not (0 <= n < CRDT_NODES and 0 < v < 1 << 32):
                    raise ValueError(f"dot ({k}, {n}) -> {v} does not fit the layout")
                u[k * CRDT_NODES + n] = v
            sl = self.slots[k]
            if len(sl) != _SLOTS or not all(0 <= x < 1 << 64 for x in sl):
                raise ValueError(f"counter of key {k} does not fit 16 u64 slots")
            w[_CTR + _SLOTS * k:_CTR + _SLOTS * (k + 1)] = np.array(sl, np.uint64)
        for n, v in self.vvector.items():
            if not (0 <= n < CRDT_NODES and 0 < v < 1 << 32):
                raise ValueError(f"version vector entry {n} -> {v} does not fit the layout")
            u[_VV + n] = v
        return w

    def increments(self, key: int):
        """Key's GCounter of increments, {node: count} (None: no such key)."""
        sl = self.slots.get(key)
        return None if sl is None else {n: sl[n] for n in range(CRDT_NODES) if sl[n]}

    def decrements(self, key: int):
        sl = self.slots.get(key)
        return None if sl is None else {n: sl[CRDT_NODES + n] for n in range(CRDT_NODES) if sl[CRDT_NODES + n]}

    def get(self, key: int):
        """PNCounterMap.get: the key's value, a signed Python int (None: no such key)."""
        sl = self.slots.get(key)
        return None if sl is None else sum(sl[:CRDT_NODES]) - sum(sl[CRDT_NODES:])

    @property
    def entries(self) -> dict:
        """PNCounterMap.entries: {key: value}."""
        return {k: self.get(k) for k in sorted(self.slots)}

    def contains(self, key: int) -> bool:
        return key in self.slots

    @property
    def size(self) -> int:
        return len(self.slots)


@dataclass
class ORMultiMap:
    """One replica's ORMultiMap: per live key its key dots {node: version} and its value set -- that set's own
    version vector {node: version} and per bound value its dots {node: version}; the key set's version vector."""
    dots: dict = field(default_factory=dict)        # key -> {node: version}, live keys only
    vvector: dict = field(default_factory=dict)     # node -> version (the key set's)
    sets: dict = field(default_factory=dict)        # key -> (vvector {node: version}, {value: {node: version}})

    @classmethod
    def from_words(cls, row) -> "ORMultiMap":
        w = np.ascontiguousarray(np.asarray(row, np.uint64)[:ORMM_WORDS])
        if w.size != ORMM_WORDS:
            raise ValueError(f"an ORMultiMap replica has {ORMM_WORDS} state words, got {w.size}")
        u = w.view(np.uint32)
        if w[_TS:272].any():
            raise ValueError("the padding words 260..271 are not zero: not canonical")
        m = cls()
        for k in range(ORSET_ELEMS):
            d = {n: int(u[k * CRDT_NODES + n]) for n in range(CRDT_NODES) if u[k * CRDT_NODES + n]}
            b = u[_SET + _SET_U32 * k:_SET + _SET_U32 * (k + 1)]
            if d:
                m.dots[k] = d
                vv = {n: int(b[n]) for n in range(CRDT_NODES) if b[n]}
                vals = {}
                for v in range(ORMM_VALUES):
                    e = b[CRDT_NODES * (1 + v):CRDT_NODES * (2 + v)]
                    if e.any():
                        vals[v] = {n: int(e[n]) for n in range(CRDT_NODES) if e[n]}
                m.sets[k] = (vv, vals)
            elif b.any():
                raise ValueError(f"key {k} has no live dot but a non-zero value set: not canonical")
        m.vvector = {n: int(u[_VV + n]) for n in range(CRDT_NODES) if u[_VV + n]}
        return m

    def to_words(self) -> np.ndarray:
        w = np.zeros(ORMM_WORDS, np.uint64)
        u = w.view(np.uint32)
        if set(self.dots) != set(self.sets):
            raise ValueError("every live key has exactly one value set")

        def put(i, n, v, what):
            if not (0 <= n < CRDT_NODES and 0 < v < 1 << 32):
                raise ValueError(f"{what} {n} -> {v} does not fit the layout")
            u[i + n] = v

        for k, d in self.dots.items():
            if not 0 <= k < ORSET_ELEMS or not d:
                raise ValueError(f"key {k}: outside the 64-key universe, or without a dot")
            for n, v in d.items():
                put(k * CRDT_NODES, n, v, f"dot of key {k}")
            vv, vals = self.sets[k]
            base = _SET + _SET_U32 * k
            for n, v in vv.items():
                put(base, n, v, f"version vector entry of key {k}'s set")
            for val, e in vals.items():
                if not 0 <= val < ORMM_VALUES or not e:
                    raise ValueError(f"value {val} of key {k}: outside the 8-value universe, or without a dot")
                for n, v in e.items():
                    put(base + CRDT_NODES * (1 + val), n, v, f"dot of value {val} of key {k}")
        for n, v in self.vvector.items():
            put(_VV, n, v, "version vector entry")
        return w

    def get(self, key: int):
        """ORMultiMap.get: the key's set of value indices, a frozenset (None: no such key)."""
        s = self.sets.get(key)
        return None if s is None else frozenset(s[1])

    def get_or_else(self, key: int, default):
        s = self.get(key)
        return default if s is None else s

    @property
    def entries(self) -> dict:
        """ORMultiMap.entries: {key: frozenset of value indices}."""
        return {k: frozenset(self.sets[k][1]) for k in sorted(self.sets)}

    def contains(self, key: int) -> bool:
        """ORMultiMap.contains reads the key set (DD/ORMultiMap.scala:131)."""
        return key in self.dots

    @property
    def size(self) -> int:
        return len(self.dots)

    @property
    def is_empty(self) -> bool:
        return not self.dots
