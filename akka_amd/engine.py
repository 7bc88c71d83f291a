"""GpuEngine: the Python host over the C ABI (include/akka_gpu.h).

One GpuEngine = one rank of the actor population on one GPU.  All arrays that
cross the boundary are plain numpy buffers (u32 ids/payloads, u64 state words).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import AgxCfg, AgxStats, check

NO_SENDER = 0xFFFFFFFF


class Kind:
    """Behaviour kinds (enum agx_behavior_kind)."""
    NONE = 0
    COUNTER = 1
    RING = 2
    FANOUT = 3
    FORWARD_RR = 4
    STOP_AFTER = 5
    PINGPONG = 6
    EVEN = 7
    GCOUNTER = 8      # Replicator-style replicas (akka-distributed-data), include/akka_gpu.h "CRDT behaviours"
    PNCOUNTER = 9
    ORSET = 10
    LWWMAP = 11       # LWWMap = ORMap of LWWRegister (AGX_KIND_LWWMAP, not in the enum), "LWWMap replicas"
    PNCOUNTERMAP = 12  # PNCounterMap = ORMap of PNCounter (AGX_KIND_PNCOUNTERMAP), "PNCounterMap replicas"
    ORMULTIMAP = 13   # ORMultiMap = ORMap of ORSet (AGX_KIND_ORMULTIMAP), "ORMultiMap replicas"


CRDT_NODES = 8
ORSET_ELEMS = 64
CRDT_WORDS = {Kind.GCOUNTER: 8, Kind.PNCOUNTER: 16, Kind.ORSET: 260, Kind.LWWMAP: 356,
              Kind.PNCOUNTERMAP: 1296, Kind.ORMULTIMAP: 2576}
# delta-CRDT mode (agx_set_delta_crdt): data + envelope/selector area + delta log (include/akka_gpu.h)
DELTA_ENV_WORDS, DELTA_LOG = 12, 64
CRDT_DELTA_WORDS = {k: w + DELTA_ENV_WORDS + (DELTA_LOG * 6 if k == Kind.ORSET else 4) for k, w in CRDT_WORDS.items()
                    if k not in (Kind.LWWMAP, Kind.PNCOUNTERMAP, Kind.ORMULTIMAP)}  # (map replicas gossip their full state only)
# LWWMap delta replication (agx_set_lwwmap_delta): data + envelope/selector area + a ring of 64 entries of 16 u32
LWWMAP_DELTA_LOG_U32 = 16
LWWMAP_DELTA_WORDS = CRDT_WORDS[Kind.LWWMAP] + DELTA_ENV_WORDS + DELTA_LOG * LWWMAP_DELTA_LOG_U32 // 2  # AGX_LWWMAP_DELTA_WORDS = 880
DELTA_MAX_SIZE = 50  # AGX_DELTA_MAX_SIZE
LWW_VALUE_MAX = 0x3FFFF
PNCMAP_COUNT_MAX = 0x3FFFF  # AGX_PNCMAP_COUNT_MAX
ORMM_VALUES = 8             # AGX_ORMM_VALUES: the value universe of an ORMultiMap key's set
LWW_CLOCKS = {"default": 0, "reverse": 1}  # AGX_LWW_CLOCK_DEFAULT / AGX_LWW_CLOCK_REVERSE
DELTA_WRITE = 0x800000
WIDE_BIT = 0x80000000


class Op:
    """Control-tell opcodes of the CRDT kinds: payload = (op << 24) | arg."""
    INCREMENT = 1
    DECREMENT = 2
    ADD = 3
    REMOVE = 4
    CLEAR = 5
    GOSSIP = 6
    DELTA_TICK = 7
    PUT = 8
    REMOVE_BINDING = 9
    REPLACE_BINDING = 10

    @staticmethod
    def make(op: int, arg: int = 0) -> int:
        return ((op & 0xFF) << 24) | (arg & 0xFFFFFF)

    @staticmethod
    def put(key: int, value: int) -> int:
        """LWWMap.put(key, value) on an LWWMap replica: key < 64, value < 2^18 (AGX_OP_PUT_ARG)."""
        if not 0 <= key < ORSET_ELEMS:
            raise ValueError(f"LWWMap key {key} outside the 64-key universe")
        if not 0 <= value <= LWW_VALUE_MAX:
            raise ValueError(f"LWWMap value {value} does not fit 18 bits")
        return Op.make(Op.PUT, key | (value << 6))

    @staticmethod
    def _count(op: int, key: int, n: int) -> int:
        if not 0 <= key < ORSET_ELEMS:
            raise ValueError(f"PNCounterMap key {key} outside the 64-key universe")
        if not 0 <= n <= PNCMAP_COUNT_MAX:
            raise ValueError(f"PNCounterMap delta {n} does not fit 18 bits (a negative delta is the other op)")
        return Op.make(op, key | (n << 6))

    @staticmethod
    def increment_key(key: int, n: int = 1) -> int:
        """PNCounterMap.increment(key, n) on a PNCounterMap replica: key < 64, 0 <= n < 2^18 (AGX_OP_COUNT_ARG)."""
        return Op._count(Op.INCREMENT, key, n)

    @staticmethod
    def decrement_key(key: int, n: int = 1) -> int:
        """PNCounterMap.decrement(key, n) on a PNCounterMap replica: key < 64, 0 <= n < 2^18 (AGX_OP_COUNT_ARG)."""
        return Op._count(Op.DECREMENT, key, n)


    @staticmethod
    def _binding(key: int, *values: int) -> None:
        if not 0 <= key < ORSET_ELEMS:
            raise ValueError(f"ORMultiMap key {key} outside the 64-key universe")
        for v in values:
            if not 0 <= v < ORMM_VALUES:
                raise ValueError(f"ORMultiMap value {v} outside the {ORMM_VALUES}-value universe")

    @staticmethod
    def add_binding(key: int, value: int) -> int:
        """ORMultiMap.addBinding(key, value) on an ORMultiMap replica: key < 64, value < 8 (AGX_OP_BINDING_ARG)."""
        Op._binding(key, value)
        return Op.make(Op.ADD, key | (value << 6))

    @staticmethod
    def remove_binding(key: int, value: int) -> int:
        """ORMultiMap.removeBinding(key, value): a set left empty takes its key with it (AGX_OP_BINDING_ARG)."""
        Op._binding(key, value)
        return Op.make(Op.REMOVE_BINDING, key | (value << 6))

    @staticmethod
    def put_set(key: int, values) -> int:
        """ORMultiMap.put(key, set): `values` is an iterable of value indices < 8, possibly empty (AGX_OP_PUT_SET_ARG)."""
        values = list(values)
        Op._binding(key, *values)
        mask = 0
        for v in values:
            mask |= 1 << v
        return Op.make(Op.PUT, key | (mask << 6))

    @staticmethod
    def replace_binding(key: int, old: int, new: int) -> int:
        """ORMultiMap.replaceBinding(key, old, new): nothing at all when old == new (AGX_OP_REPLACE_ARG)."""
        Op._binding(key, old, new)
        return Op.make(Op.REPLACE_BINDING, key | (old << 6) | (new << 9))


@dataclass
class EngineConfig:
    n_actors: int
    throughput: int = 5          # akka.actor.default-dispatcher.throughput (reference.conf:541)
    capacity: int = 0            # bounded mailbox capacity, 0 = unbounded
    n_words: int = 2
    max_emit: int = 1
    n_ranks: int = 1
    rank: int = 0
    num_shards: int = 1000
    device: int = 0
    msg_capacity: int = 0
    bucket_actors: int = 0       # actors per apply bucket (0 = 2048; power of two in [32, 2048])

    def to_c(self) -> AgxCfg:
        c = AgxCfg()
        c.abi_version = _lib.ABI_VERSION
        c.device = self.device
        c.n_actors = self.n_actors
        # throughput <= 0 behaves as 1 (Mailbox.scala:261); keep the value, the engine clamps
        c.throughput = max(int(self.throughput), 0) & 0xFFFFFFFF
        c.capacity = int(self.capacity)
        c.n_words = int(self.n_words)
        c.max_emit = int(self.max_emit)
        c.n_ranks = int(self.n_ranks)
        c.rank = int(self.rank)
        c.num_shards = int(self.num_shards)
        c.msg_capacity = int(self.msg_capacity)
        c.bucket_actors = int(self.bucket_actors)
        return c


@dataclass
class Stats:
    delivered: int = 0
    dead_letters: int = 0
    unhandled: int = 0
    emitted: int = 0
    staged: int = 0
    supersteps: int = 0
    in_flight: int = 0
    bytes_alg: int = 0

    @classmethod
    def from_c(cls, s: AgxStats) -> "Stats":
        return cls(**s.as_dict())


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def priority_table(table) -> np.ndarray:
    """256 u8 priorities by message tag from bytes or any sequence of 256 integers in [0, 255]."""
    t = np.frombuffer(bytes(table), np.uint8) if isinstance(table, (bytes, bytearray)) else np.asarray(table)
    if t.shape != (256,) or (np.asarray(t, np.int64) < 0).any() or (np.asarray(t, np.int64) > 255).any():
        raise ValueError("a mailbox priority table is 256 values in [0, 255], one per message tag")
    return np.ascontiguousarray(t.astype(np.uint8))


def _ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(ctypes.POINTER(ty))


class GpuEngine:
    """One rank of the batched dispatcher.  Mirrors agx_* one to one."""

    def __init__(self, cfg: EngineConfig):
        self.lib = _lib.load()
        self.cfg = cfg
        h = ctypes.c_void_p()
        c = cfg.to_c()
        check(self.lib.agx_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            check(self.lib.agx_destroy(self._h))
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    # -- registration
    def register_range(self, first: int, count: int, kind: int, init_state=None) -> None:
        W = self.cfg.n_words
        if init_state is None:
            check(self.lib.agx_register_range(self._h, first, count, kind, None, 0))
            return
        st = np.ascontiguousarray(np.asarray(init_state, dtype=np.uint64).reshape(count, -1))
        if st.shape[1] < W:
            st = np.concatenate([st, np.zeros((count, W - st.shape[1]), np.uint64)], axis=1)
        st = np.ascontiguousarray(st[:, :W])
        check(self.lib.agx_register_range(self._h, first, count, kind, st.ctypes.data_as(ctypes.c_void_p), W * 8))

    def set_ring(self, stride: int = 1) -> None:
        check(self.lib.agx_set_ring(self._h, stride))

    def set_mailbox_class(self, cls: int, capacity: int) -> None:
        """A further mailbox type of this dispatcher (agx_set_mailbox_class): bounded-capacity:N -> N,
        an unbounded type -> 0 (Mailboxes.lookupConfigurator, Mailboxes.scala:204-260)."""
        check(self.lib.agx_set_mailbox_class(self._h, cls, capacity))

    def set_mailbox(self, first: int, count: int, cls: int) -> None:
        """Bind actors [first, first + count) to mailbox class `cls` (agx_set_mailbox)."""
        check(self.lib.agx_set_mailbox(self._h, first, count, cls))

    def set_mailbox_priority(self, cls: int, table) -> None:
        """A priority table for mailbox class `cls` (agx_set_mailbox_priority): 256 u8, the priority of
        a message is table[payload >> 24], lower is dequeued first, equal priorities stay FIFO
        (Unbounded/BoundedStablePriorityMailbox, Mailbox.scala:726-816; a control-aware mailbox is the
        table 0 / 1, Mailbox.scala:867-1025).  None clears the table (FIFO)."""
        if table is None:
            check(self.lib.agx_set_mailbox_priority(self._h, cls, None))
            return
        t = priority_table(table)
        check(self.lib.agx_set_mailbox_priority(self._h, cls, _ptr(t, ctypes.c_uint8)))

    def set_stash(self, cls: int, capacity: int) -> None:
        """A stash of `capacity` (1..255) messages for every actor of mailbox class `cls` (agx_set_stash): the
        class is a deque-based mailbox (Unbounded/BoundedDequeBasedMailbox, classic `stash-capacity`), its
        actors' compiled behaviours may stash and unstash_all (typed.Behaviors.with_stash; StashBuffer,
        TY/internal/StashBufferImpl.scala:61-79,131-218)."""
        check(self.lib.agx_set_stash(self._h, cls, capacity))

    def stash_info(self) -> dict:
        """agx_stash_info: totals stashed / unstashed / overflows, and the messages held / pending now."""
        v = [ctypes.c_uint64() for _ in range(5)]
        check(self.lib.agx_stash_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("stashed", "unstashed", "overflows", "held", "pending"), (int(x.value) for x in v)))

    def read_stash(self, actor_id: int, cap: int = 255):
        """agx_read_stash: (senders, payloads, released) -- one actor's stash buffer in order and how
        many of its first entries are released."""
        s, p = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        rel, n = ctypes.c_uint32(), ctypes.c_uint32()
        check(self.lib.agx_read_stash(self._h, actor_id, _ptr(s, ctypes.c_uint32), _ptr(p, ctypes.c_uint32), cap,
                                      ctypes.byref(rel), ctypes.byref(n)))
        k = min(int(n.value), cap)
        return s[:k], p[:k], int(rel.value)

    def read_kinds(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """agx_read_kinds: each actor's behaviour kind now (become / unstash_all change it)."""
        if count is None:
            count = self.cfg.n_actors - first
        k = np.zeros(count, np.uint8)
        check(self.lib.agx_read_kinds(self._h, first, count, _ptr(k, ctypes.c_uint8)))
        return k

    def set_timers(self, n_keys: int) -> None:
        """`n_keys` (1..4) timer slots for every actor (agx_set_timers): Behaviors.withTimers / TimerScheduler
        (TY/internal/TimerSchedulerImpl.scala:61-172) in logical time -- one superstep is one tick.  Compiled
        behaviours may start, cancel and test timers (typed.Behaviors.with_timers)."""
        check(self.lib.agx_set_timers(self._h, n_keys))

    def start_timers(self, first: int, count: int, key: int, delay: int = 1, *, periodic: bool = False, delays=None,
                     payload: int = 0) -> None:
        """agx_start_timers: start timer `key` of actors [first, first + count) at the current tick (a withTimers
        setup block).  The first fire comes after `delay` ticks, or after `delays[i]` for actor first + i
        (staggered phases); a periodic timer's period is `delay` either way."""
        d = None
        if delays is not None:
            d = np.ascontiguousarray(delays, np.uint32)
            if d.size != count:
                raise ValueError("delays must hold one delay per actor of the range")
        check(self.lib.agx_start_timers(self._h, first, count, key, 1 if periodic else 0, int(delay),
                                        _ptr(d, ctypes.c_uint32) if d is not None else None, int(payload) & 0xFFFFFFFF))

    def timer_info(self) -> dict:
        """agx_timer_info: totals fired / discarded, the slots active / pending now, and the ticks that ran while
        the engine was not quiescent."""
        v = [ctypes.c_uint64() for _ in range(5)]
        check(self.lib.agx_timer_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("fired", "discarded", "active", "pending", "ticks"), (int(x.value) for x in v)))

    def read_timers(self, actor_id: int) -> dict:
        """agx_read_timers: one actor's four slots -- active, remaining (ticks to the next fire, 0xFFFFFFFF when
        none is to come), period, payload, generation."""
        a = [np.zeros(4, np.uint32) for _ in range(5)]
        check(self.lib.agx_read_timers(self._h, actor_id, *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(zip(("active", "remaining", "period", "payload", "generation"), a))

    def set_receive_timeout(self, transparent_tags=()) -> None:
        """Receive timeouts for every actor (agx_set_receive_timeout): context.setReceiveTimeout /
        cancelReceiveTimeout (AA/dungeon/ReceiveTimeout.scala:18-74) on top of the timers -- call set_timers first.
        Messages whose tag is in `transparent_tags` are NotInfluenceReceiveTimeout."""
        mask = np.zeros(8, np.uint32)
        for t in transparent_tags:
            if not 0 <= int(t) <= 0xFF:
                raise ValueError("a message tag has 8 bits")
            mask[int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
        check(self.lib.agx_set_receive_timeout(self._h, _ptr(mask, ctypes.c_uint32)))

    def start_receive_timeout(self, first: int, count: int, delay: int, payload: int = 0) -> None:
        """agx_start_receive_timeout: every live actor of [first, first + count) sets (delay, payload) at the
        current tick (a setup block); delay 0 cancels."""
        check(self.lib.agx_start_receive_timeout(self._h, first, count, int(delay), int(payload) & 0xFFFFFFFF))

    def receive_timeout_info(self) -> dict:
        """agx_receive_timeout_info: totals fired / discarded, the actors with a timeout set / pending now."""
        v = [ctypes.c_uint64() for _ in range(4)]
        check(self.lib.agx_receive_timeout_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("fired", "discarded", "set", "pending"), (int(x.value) for x in v)))

    def read_receive_timeout(self, first: int = 0, count: int | None = None) -> dict:
        """agx_read_receive_timeout: delay, remaining (ticks to the next fire, 0xFFFFFFFF when none is to come) and
        payload of the actors [first, first + count)."""
        count = self.cfg.n_actors - first if count is None else count
        a = [np.zeros(count, np.uint32) for _ in range(3)]
        check(self.lib.agx_read_receive_timeout(self._h, first, count, *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(zip(("delay", "remaining", "payload"), a))

    ENTITY_TYPE = np.dtype([("first_id", "<u4"), ("count", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("base0", "<u8"),
                            ("word1", "<u8"), ("stop_payload", "<u4"), ("idle_delay", "<u4"), ("idle_payload", "<u4"),
                            ("reserved", "<u4")])

    def set_sharding(self, types) -> None:
        """Sharded entities (agx_set_sharding; akka-cluster-sharding Shard.scala:388-516) on top of
        receive timeouts -- call set_timers and set_receive_timeout first.  `types` are (first_id, count, kind, word-0
        base, word-1 constant or None for the entity's id, stop payload, idle delay, idle payload),
        typed.Tables.entity_types has them: the ids of a range are unregistered, an entity starts on its first
        message, and compiled behaviours may context.passivate()."""
        t = np.zeros(max(len(types), 1), self.ENTITY_TYPE)
        for i, (first, count, kind, base, w1, stop, delay, idle) in enumerate(types):
            t[i] = (int(first), int(count), int(kind), 1 if w1 is None else 0, int(base), 0 if w1 is None else int(w1),
                    int(stop) & 0xFFFFFFFF, int(delay), int(idle) & 0xFFFFFFFF, 0)
        check(self.lib.agx_set_sharding(self._h, t.ctypes.data_as(ctypes.c_void_p), len(types)))

    SHARDING_INFO = ("started", "restarted", "passivations", "passivated", "passivate_ignored", "passivate_unknown", "alive")

    def sharding_info(self) -> dict:
        """agx_sharding_info: totals started / restarted / passivations / passivated / passivate_ignored /
        passivate_unknown, and the entities alive now."""
        v = [ctypes.c_uint64() for _ in range(7)]
        check(self.lib.agx_sharding_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.SHARDING_INFO, (int(x.value) for x in v)))

    def read_entities(self, first: int = 0, count: int | None = None) -> dict:
        """agx_read_entities: alive, incarnations and passivating of the ids [first, first + count)."""
        count = self.cfg.n_actors - first if count is None else count
        a = [np.zeros(count, np.uint32) for _ in range(3)]
        check(self.lib.agx_read_entities(self._h, first, count, *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(zip(("alive", "incarnations", "passivating"), a))

    def set_ask(self) -> None:
        """The ask pattern for every actor (agx_set_ask): context.ask -- request-response with a timeout
        (TY/internal/ActorContextImpl.scala:203-218, TY/scaladsl/AskPattern.scala:109-162) on top of
        the timers -- call set_timers first.  An ask takes one of the actor's timer keys."""
        check(self.lib.agx_set_ask(self._h))

    def ask_info(self) -> dict:
        """agx_ask_info: totals asked / answered / timed_out / late."""
        v = [ctypes.c_uint64() for _ in range(4)]
        check(self.lib.agx_ask_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("asked", "answered", "timed_out", "late"), (int(x.value) for x in v)))

    def read_asks(self, actor_id: int) -> dict:
        """agx_read_asks: per timer key, is the slot active as an ask's timeout, and its adapt tag (0xFFFFFFFF: none)."""
        a = [np.zeros(4, np.uint32) for _ in range(2)]
        check(self.lib.agx_read_asks(self._h, actor_id, *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(zip(("is_ask", "adapt"), a))

    def set_death_watch(self, n_slots: int) -> None:
        """`n_slots` (1..4) watch slots for every actor (agx_set_death_watch): context.watch / watchWith / unwatch
        and the Terminated signal (AA/dungeon/DeathWatch.scala:19-113) in the timers' logical time.  Compiled
        behaviours may watch, unwatch and handle the signal (typed.context, ReceiveBuilder.on_signal)."""
        check(self.lib.agx_set_death_watch(self._h, n_slots))

    def start_watch(self, first: int, count: int, watchees=None, *, offset: int = 0, message: int | None = None) -> None:
        """agx_start_watch: actor first + i watches watchees[i], or (first + i + offset) mod n without the array (a
        setup block, before the first run or between runs); `message`: watchWith's custom message payload."""
        w = None
        if watchees is not None:
            w = np.ascontiguousarray(watchees, np.uint32)
            if w.size != count:
                raise ValueError("watchees must hold one id per actor of the range")
        check(self.lib.agx_start_watch(self._h, first, count, _ptr(w, ctypes.c_uint32) if w is not None else None,
                                       int(offset), 0 if message is None else 1,
                                       0 if message is None else int(message) & 0xFFFFFFFF))

    WATCH_INFO = ("watches", "terminated", "discarded", "death_pacts", "conflicts", "watching", "pending", "ticks")

    def watch_info(self) -> dict:
        """agx_watch_info: totals watches / terminated / discarded / death_pacts / conflicts, the slots watching /
        pending (due) now, and the ticks that ran while the engine was active."""
        v = [ctypes.c_uint64() for _ in range(8)]
        check(self.lib.agx_watch_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.WATCH_INFO, (int(x.value) for x in v)))

    def read_watch(self, actor_id: int) -> dict:
        """agx_read_watch: one actor's four slots -- watchee, state (0 free, 1 watching, 2 due, 3 notified, | 4 with
        a custom message), payload, generation."""
        a = [np.zeros(4, np.uint32) for _ in range(4)]
        check(self.lib.agx_read_watch(self._h, actor_id, *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(zip(("watchee", "state", "payload", "generation"), a))

    def set_supervision(self, rows) -> None:
        """agx_set_supervision: `rows[b]` are compiled behaviour b's supervisor entries (typed.AgxSupervisor, inner
        first, at most 4; typed.Tables.supervisors has them): Behaviors.supervise(..).onFailure(strategy)
        (TY/internal/Supervision.scala:43-52,311-406).  Compiled cases may then end in Behaviors.throw(exc), and
        PreRestart / PostStop signal cases run."""
        from .typed import AgxSupervisor
        rows = [list(r) for r in rows]
        n_levels = max([len(r) for r in rows] + [1])  # (a row without entries: no supervisor, every failure stops)
        arr = (AgxSupervisor * max(len(rows) * n_levels, 1))()
        for b, r in enumerate(rows):
            for k, s in enumerate(r):
                arr[b * n_levels + k] = s
        check(self.lib.agx_set_supervision(self._h, ctypes.cast(arr, ctypes.c_void_p), len(rows), n_levels))

    SUPERVISION_INFO = ("failures", "resumes", "restarts", "stops", "ticks")

    def supervision_info(self) -> dict:
        """agx_supervision_info: totals failures / resumes / restarts / stops, and the ticks (supersteps with mail)."""
        v = [ctypes.c_uint64() for _ in range(5)]
        check(self.lib.agx_supervision_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.SUPERVISION_INFO, (int(x.value) for x in v)))

    def read_supervision(self, actor_id: int) -> dict:
        """agx_read_supervision: one actor's initial kind and, per level, the restart count and the ticks left of
        the window (0xFFFFFFFF: no deadline)."""
        kind = ctypes.c_uint32()
        a = [np.zeros(4, np.uint32) for _ in range(2)]
        check(self.lib.agx_read_supervision(self._h, actor_id, ctypes.byref(kind), *(_ptr(x, ctypes.c_uint32) for x in a)))
        return dict(initial_kind=int(kind.value), count=a[0], remaining=a[1])

    def set_backoff(self, rows) -> None:
        """agx_set_backoff, after set_supervision: `rows[b]` are compiled behaviour b's backoff rows (typed.AgxBackoff,
        one per supervisor entry, inner first; typed.Tables.backoff has them).  A row with min_backoff != 0 turns
        the restart entry of the same place into SupervisorStrategy.restartWithBackoff (TY/internal/Supervision.
        scala:163-406); the others leave theirs a plain restart."""
        from .typed import AgxBackoff
        rows = [list(r) for r in rows]
        n_levels = max([len(r) for r in rows] + [1])
        arr = (AgxBackoff * max(len(rows) * n_levels, 1))()
        for b, r in enumerate(rows):
            for k, s in enumerate(r):
                arr[b * n_levels + k] = s
        check(self.lib.agx_set_backoff(self._h, ctypes.cast(arr, ctypes.c_void_p), len(rows), n_levels))

    BACKOFF_INFO = ("backoffs", "resumed", "dropped", "limit_stops", "suspended")

    def backoff_info(self) -> dict:
        """agx_backoff_info: totals backoffs / resumed / dropped / limit_stops, and the actors suspended now."""
        v = [ctypes.c_uint64() for _ in range(5)]
        check(self.lib.agx_backoff_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.BACKOFF_INFO, (int(x.value) for x in v)))

    def read_backoff(self, actor_id: int) -> dict:
        """agx_read_backoff: the coming ticks during which the actor stays suspended (0: it drains in the next tick)
        and the tick at which it drains again (0: never suspended)."""
        v = [ctypes.c_uint32() for _ in range(2)]
        check(self.lib.agx_read_backoff(self._h, actor_id, *(ctypes.byref(x) for x in v)))
        return dict(suspended_for=int(v[0].value), until=int(v[1].value))

    def set_children(self, regions, sites) -> None:
        """agx_set_children (an engine with death watch, before the first run): `regions` are (first_parent,
        n_parents, first_child, max_children) -- the k-th spawn of parent p creates id first_child + (p -
        first_parent) * max_children + k; `sites` are (kind, word-0 base, word-1 constant or None for the parent's
        id), typed.Tables.spawn_sites has them.  Compiled behaviours may then context.spawn / context.stop."""
        r = np.ascontiguousarray(np.asarray(list(regions), np.uint32).reshape(-1, 4))
        st = np.zeros(max(len(sites), 1), np.dtype([("kind", "<u4"), ("flags", "<u4"), ("base0", "<u8"), ("word1", "<u8")]))
        for i, (kind, base, w1) in enumerate(sites):
            st[i] = (int(kind), 1 if w1 is None else 0, int(base), 0 if w1 is None else int(w1))
        check(self.lib.agx_set_children(self._h, r.ctypes.data_as(ctypes.c_void_p), r.shape[0],
                                        st.ctypes.data_as(ctypes.c_void_p), len(sites)))

    def spawn_children(self, first: int, count: int, site: int, arg: int = 0) -> None:
        """agx_spawn_children: every live actor of the range spawns once from `site` (the setup block,
        Behaviors.setup { ctx => ctx.spawn(..) }); the Create arrives in the next tick."""
        check(self.lib.agx_spawn_children(self._h, first, count, site, arg))

    CHILDREN_INFO = ("spawned", "refused", "created", "child_stops", "cascade_stops", "illegal_stops", "discarded", "live")

    def children_info(self) -> dict:
        """agx_children_info: totals spawned / refused / created / child_stops / cascade_stops / illegal_stops /
        discarded, and the created children alive now."""
        v = [ctypes.c_uint64() for _ in range(8)]
        check(self.lib.agx_children_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.CHILDREN_INFO, (int(x.value) for x in v)))

    def read_children(self, actor_id: int) -> dict:
        """agx_read_children: the actor's computed parent (0xFFFFFFFF: none), its spawn count, whether it was ever
        created."""
        v = [ctypes.c_uint32() for _ in range(3)]
        check(self.lib.agx_read_children(self._h, actor_id, *(ctypes.byref(x) for x in v)))
        return dict(zip(("parent", "spawn_count", "created"), (int(x.value) for x in v)))

    def set_receptionist(self, n_keys: int, capacity: int) -> None:
        """agx_set_receptionist (before the first run, an engine of its own): `n_keys` service keys (1..8, typed
        Tables.service_keys has them), listings of at most `capacity` ids.  Compiled behaviours may then
        context.register / deregister / route / forward and read the listings."""
        check(self.lib.agx_set_receptionist(self._h, n_keys, capacity))

    def register_services(self, first: int, count: int, key: int, on: bool = True) -> None:
        """agx_register_services: the live actors of the range register under (on=False: deregister from) service
        key number `key` -- the setup block; the listing is in force for the next tick."""
        check(self.lib.agx_register_services(self._h, first, count, key, 1 if on else 0))

    def read_listing(self, key: int) -> np.ndarray:
        """agx_read_listing: the listing of key number `key` in force for the next tick, ascending ids."""
        n = ctypes.c_uint64()
        check(self.lib.agx_read_listing(self._h, key, None, 0, ctypes.byref(n)))
        out = np.zeros(max(int(n.value), 1), np.uint32)
        check(self.lib.agx_read_listing(self._h, key, _ptr(out, ctypes.c_uint32), int(n.value), ctypes.byref(n)))
        return out[:int(n.value)]

    def read_services(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """agx_read_services: the key masks (bit k = registered under key k) of actors [first, first + count)."""
        count = self.cfg.n_actors - first if count is None else count
        out = np.zeros(max(count, 1), np.uint8)
        check(self.lib.agx_read_services(self._h, first, count, _ptr(out, ctypes.c_uint8)))
        return out[:count]

    RECEPTIONIST_INFO = ("routed", "no_routees", "registered", "deregistered", "terminated", "rebuilds")

    def receptionist_info(self) -> dict:
        """agx_receptionist_info: totals routed / no_routees / registered / deregistered / terminated / rebuilds, and
        per key the size of the listing in force for the next tick and its version."""
        v = [ctypes.c_uint64() for _ in range(6)]
        size, version = np.zeros(8, np.uint32), np.zeros(8, np.uint64)
        check(self.lib.agx_receptionist_info(self._h, *(ctypes.byref(x) for x in v), _ptr(size, ctypes.c_uint32),
                                             _ptr(version, ctypes.c_uint64)))
        d = dict(zip(self.RECEPTIONIST_INFO, (int(x.value) for x in v)))
        d["size"] = [int(x) for x in size]
        d["version"] = [int(x) for x in version]
        return d

    def set_topics(self, log_capacity: int = 1024) -> None:
        """agx_set_topics (after set_receptionist, before the first run): the engine's service keys are pub-sub topics
        as well; compiled behaviours may then context.publish, at most `log_capacity` (1..65536) publications per
        tick."""
        check(self.lib.agx_set_topics(self._h, log_capacity))

    def publish(self, key: int, payload: int, sender: int = NO_SENDER) -> None:
        """agx_publish: a publication from the host to topic number `key`, delivered in the next tick to every
        subscriber, after the device's own publications of the tick before."""
        check(self.lib.agx_publish(self._h, key, sender, payload))

    TOPIC_INFO = ("published", "fanned_out", "no_subscribers", "host_published")

    def topic_info(self) -> dict:
        """agx_topic_info: totals published / fanned_out / no_subscribers / host_published."""
        v = [ctypes.c_uint64() for _ in range(4)]
        check(self.lib.agx_topic_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.TOPIC_INFO, (int(x.value) for x in v)))

    def read_topic_log(self) -> np.ndarray:
        """agx_read_topic_log: the pending log, one (key, sender, payload) row per publication, in delivery order."""
        n = ctypes.c_uint64()
        check(self.lib.agx_read_topic_log(self._h, None, None, None, 0, ctypes.byref(n)))
        k, s, p = (np.zeros(max(int(n.value), 1), np.uint32) for _ in range(3))
        check(self.lib.agx_read_topic_log(self._h, *(_ptr(x, ctypes.c_uint32) for x in (k, s, p)), int(n.value), ctypes.byref(n)))
        return np.stack([k, s, p], axis=1)[:int(n.value)]

    def set_listings(self, listing_payloads) -> None:
        """agx_set_listings (after set_topics, before the first run): compiled behaviours may then
        context.receptionist_subscribe / receptionist_find; listing_payloads[k] is the payload of a Listing envelope of
        key k, one per key of the receptionist (Tables.listing_payloads)."""
        p = np.ascontiguousarray(listing_payloads, dtype=np.uint32)
        check(self.lib.agx_set_listings(self._h, _ptr(p, ctypes.c_uint32), int(p.size)))

    def subscribe_listings(self, first: int, count: int, key: int, on: bool = True) -> None:
        """agx_subscribe_listings: the setup block -- the live actors of [first, first + count) subscribe to key
        number `key` and are owed its Listing at the next tick (on), or no longer subscribe to it (off)."""
        check(self.lib.agx_subscribe_listings(self._h, first, count, key, 1 if on else 0))

    LISTING_INFO = ("subscribes", "finds", "listings_sent", "notified")

    def listing_info(self) -> dict:
        """agx_listing_info: totals subscribes / finds / listings_sent / notified."""
        v = [ctypes.c_uint64() for _ in range(4)]
        check(self.lib.agx_listing_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(self.LISTING_INFO, (int(x.value) for x in v)))

    def read_subscriptions(self, first: int = 0, count: int | None = None):
        """agx_read_subscriptions: the (sub, pending) masks of actors [first, first + count)."""
        count = self.cfg.n_actors - first if count is None else count
        sub, pend = np.zeros(max(count, 1), np.uint8), np.zeros(max(count, 1), np.uint8)
        check(self.lib.agx_read_subscriptions(self._h, first, count, _ptr(sub, ctypes.c_uint8), _ptr(pend, ctypes.c_uint8)))
        return sub[:count], pend[:count]

    def set_router_logics(self, hashed_keys_mask: int, virtual_nodes_factor: int = 0, seed: int = 0) -> None:
        """agx_set_router_logics (after set_receptionist, before the first run; not with topics): the keys of
        `hashed_keys_mask` (typed Tables.hashed_keys_mask) get a consistent-hash ring of `virtual_nodes_factor` points
        per registered actor; `seed` seeds random routing.  Compiled behaviours may then context.route_hashed /
        route_random."""
        check(self.lib.agx_set_router_logics(self._h, hashed_keys_mask, virtual_nodes_factor, seed))

    ROUTER_INFO = ("hashed", "random", "ring_rebuilds")

    def router_info(self) -> dict:
        """agx_router_info: totals hashed / random / ring_rebuilds, and per key the size of the hash ring in force for
        the next tick (in ring points)."""
        v = [ctypes.c_uint64() for _ in range(3)]
        size = np.zeros(8, np.uint32)
        check(self.lib.agx_router_info(self._h, *(ctypes.byref(x) for x in v), _ptr(size, ctypes.c_uint32)))
        d = dict(zip(self.ROUTER_INFO, (int(x.value) for x in v)))
        d["ring_size"] = [int(x) for x in size]
        return d

    def read_hash_ring(self, key: int) -> tuple:
        """agx_read_hash_ring: (hashes, ids) of the ring of hashed key number `key` in force for the next tick, in ring
        order (the hashes as the unsigned 32-bit patterns of the signed values the ring is ordered by)."""
        n = ctypes.c_uint64()
        check(self.lib.agx_read_hash_ring(self._h, key, None, None, 0, ctypes.byref(n)))
        hs, ids = np.zeros(max(int(n.value), 1), np.uint32), np.zeros(max(int(n.value), 1), np.uint32)
        check(self.lib.agx_read_hash_ring(self._h, key, _ptr(hs, ctypes.c_uint32), _ptr(ids, ctypes.c_uint32), int(n.value),
                                          ctypes.byref(n)))
        return hs[:int(n.value)], ids[:int(n.value)]

    def set_outbound(self, first_host_id: int, n_host: int, capacity: int = 1 << 20) -> None:
        """Host-side actor ids [first_host_id, +n_host): GPU tells to them go to the outbox
        (agx_set_outbound; the reply path of sender() ! reply, ActorCell.scala:583-587)."""
        check(self.lib.agx_set_outbound(self._h, first_host_id, n_host, capacity))

    def take_outbound(self, cap: int = 1 << 24):
        """agx_take_outbound: (dst, src, payload) arrays, each sender's tells in emission order."""
        d, s, p = (np.zeros(cap, np.uint32) for _ in range(3))
        n = ctypes.c_uint64()
        check(self.lib.agx_take_outbound(self._h, _ptr(d, ctypes.c_uint32), _ptr(s, ctypes.c_uint32),
                                         _ptr(p, ctypes.c_uint32), cap, ctypes.byref(n)))
        k = int(n.value)
        return d[:k], s[:k], p[:k]

    def set_gossip(self, fanout: int, seed: int) -> None:
        check(self.lib.agx_set_gossip(self._h, fanout, seed))

    def set_behaviors(self, tables) -> None:
        """Compiled behaviours (akka_amd.typed.compile_behaviors -> agx_set_behaviors)."""
        check(self.lib.agx_set_behaviors(self._h, ctypes.addressof(tables.cases), len(tables.cases),
                                         ctypes.addressof(tables.acts), len(tables.acts),
                                         _ptr(tables.first, ctypes.c_uint32), tables.n_behaviors))

    def set_delta_crdt(self, max_delta_size: int) -> None:
        """Replicator delta-crdt.enabled / max-delta-size (0 = off)."""
        check(self.lib.agx_set_delta_crdt(self._h, max_delta_size))

    def set_lwwmap_delta(self, max_delta_size: int = DELTA_MAX_SIZE) -> None:
        """Delta replication for an LWWMap engine (ORMap.DeltaOp: PutDeltaOp / RemoveDeltaOp groups, causal delivery,
        full-state gossip as the repair path): max_delta_size 1..50; needs n_words >= LWWMAP_DELTA_WORDS and
        max_emit >= 4.  After the LWWMap replicas are registered, before the first run."""
        fn = getattr(self.lib, "agx_set_lwwmap_delta", None)
        if fn is None:
            raise RuntimeError("this libakka_gpu.so has no agx_set_lwwmap_delta (an older build)")
        check(fn(self._h, max_delta_size))

    def set_lwwmap(self, clock: str = "default", base: int = 0) -> None:
        """The LWWRegister clock of an LWWMap engine: "default" (last write wins) or "reverse" (first write
        wins), logical time base + superstep number.  After registering the replicas, before the first run."""
        if clock not in LWW_CLOCKS:
            raise ValueError(f"unknown LWWMap clock {clock!r} (one of {sorted(LWW_CLOCKS)})")
        if not 0 <= base < 1 << 64:
            raise ValueError("LWWMap clock base must be an unsigned 64-bit integer")
        check(self.lib.agx_set_lwwmap(self._h, LWW_CLOCKS[clock], base))

    def set_fanout(self, k: int, seed: int, cdf, perm) -> None:
        cdf = _u32(cdf)
        perm = _u32(perm)
        check(self.lib.agx_set_fanout(self._h, k, seed, _ptr(cdf, ctypes.c_uint32), _ptr(perm, ctypes.c_uint32),
                                      cdf.size))

    def set_graph(self, row_ptr, col) -> None:
        rp = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.uint64))
        cl = _u32(col) if len(col) else np.zeros(1, np.uint32)
        check(self.lib.agx_set_graph(self._h, _ptr(rp, ctypes.c_uint64), _ptr(cl, ctypes.c_uint32)))

    def set_graph_rmat(self, row_ptr, bits: int, ta: int, tb: int, tc: int, seed: int) -> None:
        """CSR rows from the host, R-MAT destinations generated on the device."""
        rp = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.uint64))
        check(self.lib.agx_set_graph_rmat(self._h, _ptr(rp, ctypes.c_uint64), bits, ta, tb, tc, seed))

    # -- tell / run
    def tell(self, dst, payload, src=None) -> None:
        dst = _u32(dst)
        pay = _u32(np.broadcast_to(np.asarray(payload, dtype=np.uint32), dst.shape))  # (a scalar: every tell)
        srcp = None
        if src is not None:
            s = _u32(np.broadcast_to(np.asarray(src, dtype=np.uint32), dst.shape))
            srcp = _ptr(s, ctypes.c_uint32)
        check(self.lib.agx_stage_tells(self._h, _ptr(dst, ctypes.c_uint32), srcp, _ptr(pay, ctypes.c_uint32),
                                       dst.size))

    def tell_one(self, dst: int, payload: int, src: int = NO_SENDER) -> bool:
        """agx_tell (any thread, lock-free): True iff the caller must submit the pump (the engine
        went from idle to scheduled)."""
        sched = ctypes.c_int32(0)
        check(self.lib.agx_tell(self._h, dst, src, payload, ctypes.byref(sched)))
        return bool(sched.value)

    def pump_idle(self) -> bool:
        """agx_pump_idle (the pump's last call): True iff the pump must be submitted again -- tells
        arrived meanwhile or wait for capacity, or the last run left mail in flight."""
        again = ctypes.c_int32(0)
        check(self.lib.agx_pump_idle(self._h, ctypes.byref(again)))
        return bool(again.value)

    def pump_cancel(self) -> None:
        """agx_pump_cancel: the pump could not be submitted; back to idle without the re-check."""
        check(self.lib.agx_pump_cancel(self._h))

    def run(self, max_supersteps: int = 1 << 30, stats: bool = True) -> Stats | None:
        """agx_run.  stats=False skips the counter read-back (read them with stats()).  On an engine with timers
        a superstep is a tick and a periodic timer never lets the engine go quiescent: always pass a budget."""
        if not stats:
            check(self.lib.agx_run(self._h, min(int(max_supersteps), 0xFFFFFFFF), None))
            return None
        st = AgxStats()
        check(self.lib.agx_run(self._h, min(int(max_supersteps), 0xFFFFFFFF), ctypes.byref(st)))
        return Stats.from_c(st)

    def run_timed(self, max_supersteps: int) -> tuple:
        """agx_run_timed: (stats, device ms of the run: HIP events on the engine stream)."""
        st = AgxStats()
        ms = ctypes.c_float()
        check(self.lib.agx_run_timed(self._h, min(int(max_supersteps), 0xFFFFFFFF), ctypes.byref(st), ctypes.byref(ms)))
        return Stats.from_c(st), float(ms.value)

    def identity_supersteps(self) -> int:
        """Multi-pass supersteps grouped without a radix pass (agx_identity_supersteps)."""
        v = ctypes.c_uint64()
        check(self.lib.agx_identity_supersteps(self._h, ctypes.byref(v)))
        return int(v.value)

    def ring_buckets(self) -> int:
        """Buckets whose queued messages live in bounded-mailbox rings (agx_ring_buckets)."""
        v = ctypes.c_uint64()
        check(self.lib.agx_ring_buckets(self._h, ctypes.byref(v)))
        return v.value

    def exchange_info(self) -> dict:
        """This rank's multi-rank exchange accounting (agx_exchange_info)."""
        v = (ctypes.c_uint64 * 6)()
        check(self.lib.agx_exchange_info(self._h, v))
        return {"dev_steps": v[0], "host_steps": v[1], "env_bytes": v[2], "row_bytes": v[3],
                "rows_on_host": bool(v[4]), "slab": v[5]}

    def persist_info(self) -> dict:
        """Replays run as one persistent launch and their supersteps (agx_persist_info)."""
        v = (ctypes.c_uint64 * 2)()
        check(self.lib.agx_persist_info(self._h, v))
        return {"launches": v[0], "supersteps": v[1]}

    def stats(self) -> Stats:
        st = AgxStats()
        check(self.lib.agx_get_stats(self._h, ctypes.byref(st)))
        return Stats.from_c(st)

    def read_state(self, first: int = 0, count: int | None = None):
        if count is None:
            count = self.cfg.n_actors - first
        W = self.cfg.n_words
        words = np.zeros((count, W), np.uint64)
        alive = np.zeros(count, np.uint8)
        check(self.lib.agx_read_state(self._h, first, count, _ptr(words, ctypes.c_uint64),
                                      _ptr(alive, ctypes.c_uint8)))
        return words, alive

    # -- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _lib.load()
        buf = (ctypes.c_uint8 * 128)()
        check(lib.agx_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid: bytes) -> None:
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(self.lib.agx_comm_init(self._h, buf))

    @staticmethod
    def group_run(engines: list["GpuEngine"], max_supersteps: int = 1 << 30) -> Stats:
        lib = _lib.load()
        arr = (ctypes.c_void_p * len(engines))(*[e._h.value for e in engines])
        st = AgxStats()
        check(lib.agx_group_run(arr, len(engines), min(int(max_supersteps), 0xFFFFFFFF), ctypes.byref(st)))
        return Stats.from_c(st)

    # -- measurement
    def profile(self, on: bool = True) -> None:
        check(self.lib.agx_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self) -> None:
        check(self.lib.agx_profile_reset(self._h))

    def profile_read(self) -> dict:
        cap = 16
        names = (ctypes.c_char * 32 * cap)()
        ms = (ctypes.c_double * cap)()
        launches = (ctypes.c_uint64 * cap)()
        items = (ctypes.c_uint64 * cap)()
        n = ctypes.c_uint32()
        check(self.lib.agx_profile_read(self._h, names, ms, launches, items, cap, ctypes.byref(n)))
        out = {}
        for i in range(min(n.value, cap)):
            out[bytes(names[i]).split(b"\0")[0].decode()] = {"total_ms": ms[i], "launches": int(launches[i]),
                                                             "items": int(items[i])}
        return out


def shard_id(entity_id: int, num_shards: int = 1000) -> int:
    """HashCodeMessageExtractor.shardId for a numeric entity id (native helper)."""
    return int(_lib.load().agx_shard_id(entity_id, num_shards))


def owner(entity_id: int, num_shards: int, n_ranks: int) -> int:
    return int(_lib.load().agx_owner(entity_id, num_shards, n_ranks))


MR_GO, MR_OVER_SLAB, MR_QUIET, MR_OVER_CAPACITY = 0, 1, 2, 3


def mr_plan(mat, rank: int, slab: int, cap: int) -> dict:
    """agx_mr_plan: the device-resident replays' decision for one superstep (the same code as
    k_mr_pack): code (MR_*), this rank's send / receive offsets (R + 1 each) and backlog."""
    m = np.ascontiguousarray(np.asarray(mat, dtype=np.uint64))
    R = m.shape[0]
    so, ro = np.zeros(R + 1, np.uint64), np.zeros(R + 1, np.uint64)
    code, nbl = ctypes.c_uint32(), ctypes.c_uint64()
    check(_lib.load().agx_mr_plan(_ptr(m, ctypes.c_uint64), R, rank, slab, cap, ctypes.byref(code),
                                  _ptr(so, ctypes.c_uint64), _ptr(ro, ctypes.c_uint64), ctypes.byref(nbl)))
    return {"code": int(code.value), "send_off": so, "recv_off": ro, "n_backlog": int(nbl.value)}


def mr_initial_slab(n_global: int, max_emit: int, R: int) -> int:
    """The first slab size of the device-resident replays (agx_engine.hip mr_initial_slab)."""
    share = n_global * max_emit // (R * R)
    return min(share + share // 4 + 1024, 1 << 30)


def exchange_plan(mat, rank: int) -> dict:
    """agx_exchange_plan: this rank's send/recv counts and offsets (host only)."""
    m = np.ascontiguousarray(np.asarray(mat, dtype=np.uint64))
    R = m.shape[0]
    out = {k: np.zeros(R, np.uint64) for k in ("send_cnt", "send_off", "recv_cnt", "recv_off")}
    infl = ctypes.c_uint64()
    check(_lib.load().agx_exchange_plan(_ptr(m, ctypes.c_uint64), R, rank, *(_ptr(out[k], ctypes.c_uint64) for k in
                                                                          ("send_cnt", "send_off", "recv_cnt",
                                                                           "recv_off")), ctypes.byref(infl)))
    out["inflight"] = int(infl.value)
    return out
