"""Typed behaviours lowered to compiled behaviour tables.

A subset of the typed actor DSL -- ``Behaviors.receiveMessage`` / ``Behaviors.same`` /
``Behaviors.stopped`` / ``Behaviors.unhandled`` (akka-actor-typed/src/main/scala/akka/actor/typed/
scaladsl/Behaviors.scala:101-121) and the javadsl ``ReceiveBuilder`` (onMessage / onMessageEquals /
onAnyMessage, akka-actor-typed/src/main/scala/akka/actor/typed/javadsl/ReceiveBuilder.scala:48-98)
-- is written here against symbolic messages and state, and lowered to the engine's case/action
tables (include/akka_gpu.h "compiled behaviours", ``agx_set_behaviors``).  The engine (and the
oracle) then run every actor registered with ``kind_of(behavior)`` through those tables:
ReceiveBuilder.receive's first-matching-handler rule (:209-218), ``Behaviors.unhandled`` when no
handler matches, and ``become`` when a handler returns another behaviour (TY/Behavior.scala:150,
ActorAdapter.next TY/internal/adapter/ActorAdapter.scala:152-168).

What lowers:
  * messages are u32 payloads; a ``MessageType`` owns a tag (payload >> 24) and carries a 24-bit
    argument, ``m.payload`` / ``m.tag`` / ``m.arg`` / ``m.sender`` are the message's fields;
  * state is at most two u64 fields (the actor's state words 0 and 1);
  * ``Behaviors.with_stash(capacity, lambda buffer: ...)`` (TY/scaladsl/Behaviors.scala withStash; StashBuffer,
    TY/internal/StashBufferImpl.scala): ``buffer.stash()`` as a case's last effect keeps the message,
    ``buffer.unstash_all(behavior)`` as its result releases the buffered messages into `behavior`,
    ``buffer.size`` / ``is_empty`` / ``is_full`` are usable in tests and values; the actors' mailbox class
    carries the capacity (``Tables.stash_capacity`` -> engine.set_stash);
  * ``Behaviors.supervise(behavior, reset={field: value}).on_failure(strategy, exc=...)`` (TY/internal/
    Supervision.scala:43-52,311-406), nestable, with ``SupervisorStrategy.resume / stop / restart /
    restart.with_limit(n, within)``; a case may end in ``Behaviors.throw(exc)``, ``ExceptionType(name, parent)``
    declares the classes, and ``on_signal(PreRestart | PostStop, ...)`` handles the two signals
    (``Tables.supervisors`` -> engine.set_supervision);
  * ``SupervisorStrategy.restart_with_backoff(min_backoff, max_backoff, random_factor)`` with
    ``.with_max_restarts(n)``, ``.with_reset_backoff_after(ticks)`` and ``.with_stash_capacity(n)`` (TY/internal/
    Supervision.scala:163-406): times are ticks (``Tables.backoff`` -> engine.set_backoff, after
    engine.set_supervision; ``Tables.uses_backoff``);
  * ``context.spawn(behavior, arg, word1=<const> | context.PARENT, into=field)``, ``context.stop(child)``,
    ``context.child_at(x)`` and ``context.spawned`` (children on the death-watch engine): the
    spawned behaviours are lowered with their parents, ``Tables.spawn_sites`` goes to engine.set_children, and a
    case holds at most one of tell, spawn and stop;
  * ``context.set_receive_timeout(delay, msg)`` and ``context.cancel_receive_timeout()`` (receive timeouts on the
    timers engine); ``compile_behaviors(..., transparent=(MessageType, ...))`` names the
    NotInfluenceReceiveTimeout types (``Tables.transparent_tags`` -> engine.set_receive_timeout, after
    engine.set_timers(max(Tables.timer_keys, 1)));
  * ``ServiceKey(name)``, ``context.register(key)`` / ``deregister(key)``, ``context.listing_size(key)``,
    ``context.service_at(key, x)``, ``context.route(key, msg, cursor=field)`` / ``route_by(key, index, msg)``,
    ``ref.forward(msg)`` and ``Routers.group(key)`` (the receptionist and group routers): keys are
    numbered in order of first appearance (``Tables.service_keys`` -> engine.set_receptionist), and a case holds at
    most one of tell and route;
  * ``context.ask(ref, msg, timeout, on_timeout=msg, on_success=MessageType | None, key=None)`` and
    ``context.ask_pending(key)`` inside ``Behaviors.with_timers`` (the ask pattern on the timers engine, DESIGN.md
    §2.9): an ask takes a timer key and lowers to ``A_ASK_ARM`` + ``A_ASK_SEND``; ``Tables.uses_ask`` ->
    engine.set_ask(), after engine.set_timers(Tables.timer_keys);
  * ``Topic(name)``, ``context.subscribe(topic)`` / ``unsubscribe(topic)``, ``context.publish(topic, msg)`` and
    ``context.subscriber_count(topic)`` (pub-sub topics on the receptionist's engine): a topic is
    numbered with the ServiceKeys, subscribing lowers to ``A_REGISTER``, and a case holds at most one of tell, route
    and publish; ``Tables.uses_topics`` -> engine.set_topics(log_capacity), after engine.set_receptionist;
  * ``context.receptionist_subscribe(key, ListingMsg)`` / ``context.receptionist_find(key, ListingMsg)``
    (Receptionist.Subscribe / Find and the Listing message): ``A_SUBSCRIBE_LISTING`` / ``A_FIND``
    with the key as pad1; the Listing of key k arrives as ``ListingMsg(k)``, one message type per key, and its
    handler reads ``context.listing_size(key)`` / ``service_at(key, x)``; ``Tables.uses_listings`` ->
    engine.set_listings(tables.listing_payloads), after engine.set_topics;
  * ``context.route_hashed(key, hash_key, msg)`` / ``context.route_random(key, msg, counter=field)`` and
    ``Routers.group(key).with_consistent_hash_routing(factor, mapping)`` / ``.with_random_routing()`` (DESIGN.md
    §2.12): ``A_ROUTE`` with ``ROUTE_HASHED`` / ``ROUTE_RANDOM``; ``Tables.uses_router_logics`` ->
    engine.set_router_logics(tables.hashed_keys_mask, tables.virtual_nodes_factor, seed), after
    engine.set_receptionist; not together with topics or listings;
  * ``EntityTypeKey(name)``, ``Entity(key, behavior, first_id, count, word0=.., word1=.. | Entity.ID)
    .with_stop_message(msg).with_receive_timeout(delay, msg)`` and ``context.passivate()`` (sharded entities on the
    receive-timeout engine): ``compile_behaviors(..., entities=[...])`` lowers the entities'
    behaviours with the roots, ``Tables.entity_types`` goes to engine.set_sharding after engine.set_receive_timeout,
    refs to entities are ordinary ids, and a case holds at most one of tell and passivate;
  * a handler returns a list of effects -- ``field.set/add/inc/max/min(v)``, ``ref.tell(v)`` --
    followed by the next behaviour; ``test=`` (a message predicate, like ReceiveBuilder's
    ``JPredicate``) and ``when=`` (a state guard: the lowering of an ``if`` inside a handler into
    two handlers) give each handler at most two tests beside its message type.

    counter = (ReceiveBuilder.create(State("count", "sum"))
               .on_any_message(lambda m, s: [s.count.inc(), s.sum.add(m.payload), Behaviors.same])
               .build("counter"))
    tables = compile_behaviors([counter])     # -> engine.set_behaviors(tables)
    engine.register_range(0, n, tables.kind_of(counter))
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field, replace

import numpy as np

KIND_COMPILED = 16
MAX_BEHAVIORS, MAX_CASES, MAX_ACTS = 64, 1024, 4096

V_CONST, V_PAYLOAD, V_TAG, V_ARG, V_WORD, V_SENDER, V_SELF, V_STASH, V_TIMER = range(9)
CMP_ANY, CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(7)
A_SET, A_ADD, A_MAX, A_MIN, A_TELL = 1, 2, 3, 4, 5
A_TIMER_SINGLE, A_TIMER_PERIODIC, A_TIMER_CANCEL, A_TIMER_CANCEL_ALL = 6, 7, 8, 9
TAG_TIMER = 0xFF     # the message tag of a TimerMsg: reserved when the tables use timers
MAX_TIMER_KEYS = 4
MAX_TIMER_DELAY = (1 << 31) - 1
A_WATCH, A_WATCH_WITH, A_UNWATCH = 10, 11, 12
TAG_WATCH = 0xFE     # the message tag of a Terminated envelope: reserved when the tables use death watch
MAX_WATCH_SLOTS = 4
CASE_SIGNAL = 0x80   # agx_case.result flag: a signal case (receiveSignal)
SIGNAL_TERMINATED = 0xFE000001  # what the payload reads as inside a signal case
RES_SAME, RES_STOPPED, RES_UNHANDLED, RES_BECOME, RES_STASH, RES_UNSTASH_ALL = 0, 1, 2, 3, 4, 5
NEXT_SAME = 0xFF  # agx_case.next of RES_UNSTASH_ALL: the behaviour stays
MAX_STASH = 255
RES_FAIL = 6         # the handler throws; agx_case.next is the exception class (engines with supervision)
MAX_EXCEPTION_CLASSES = 32
MAX_SUPERVISORS = 4
SIGNAL_PRERESTART, SIGNAL_POSTSTOP = 0xFE000002, 0xFE000003
SUP_RESUME, SUP_RESTART, SUP_STOP = 1, 2, 3
V_SPAWNED, V_CHILD = 9, 10   # engines with children: the spawn count; child number (value + k) mod the spawn count
CHILD_NO_WORD = 2            # V_CHILD's `word` when the index is a constant (no state word)
A_SPAWN, A_STOP_CHILD = 13, 14
TAG_CREATE, TAG_STOP = 0xFD, 0xFC  # the tags of Create / Stop envelopes: reserved when the tables use children
MAX_CHILD_REGIONS, MAX_SPAWN_SITES = 8, 64
SPAWN_ARG_BITS = 18          # a spawn's argument: its low 18 bits are added to the site's word-0 base
A_SET_RECEIVE_TIMEOUT, A_CANCEL_RECEIVE_TIMEOUT = 15, 16
TAG_RECEIVE_TIMEOUT = 0xFB   # the tag of a receive-timeout envelope: reserved when the tables use receive timeouts
V_LISTING_SIZE, V_SERVICE_AT = 11, 12  # engines with the receptionist; `word` = key | selector << 3
SVC_WORD0, SVC_WORD1, SVC_ARG, SVC_CONST = 0, 1, 2, 3  # V_SERVICE_AT's selector: what x of listing[x mod size] is
A_REGISTER, A_DEREGISTER, A_ROUTE = 17, 18, 19     # the service key is pad1
ROUTE_KEEP_SENDER, ROUTE_BY_INDEX = 1, 2           # pad0 of A_ROUTE (KEEP_SENDER also of A_TELL: ref.forward)
ROUTE_HASHED, ROUTE_RANDOM = 4, 8                  # pad0 of A_ROUTE on an engine with router logics
MAX_VIRTUAL_NODES = 64
A_ASK_ARM, A_ASK_SEND = 20, 21                     # context.ask: `word` is the timer key
A_PUBLISH = 22                                     # context.publish: the topic's key is pad1
A_SUBSCRIBE_LISTING, A_FIND = 23, 24               # context.receptionist_subscribe / _find: the key is pad1
# the ask ref a target sees as the sender: ASK_REF_BIT | key << 29 | (generation mod 2^7) << 22 | the asker's id
ASK_REF_BIT, ASK_REF_KEY_SHIFT, ASK_REF_GEN_SHIFT, ASK_REF_GEN_MASK, ASK_REF_ID_MASK = 1 << 31, 29, 22, 0x7F, (1 << 22) - 1
ASK_MAX_ACTORS = (1 << 22) - 1
MAX_SERVICE_KEYS = 8
A_PASSIVATE = 25                                   # context.passivate: shard ! Passivate(self)
MAX_ENTITY_TYPES = 8


class AgxCase(ctypes.Structure):
    """include/akka_gpu.h agx_case (48 B)."""
    _fields_ = [("src1", ctypes.c_uint8), ("word1", ctypes.c_uint8), ("cmp1", ctypes.c_uint8), ("src2", ctypes.c_uint8),
                ("word2", ctypes.c_uint8), ("src3", ctypes.c_uint8), ("word3", ctypes.c_uint8), ("cmp2", ctypes.c_uint8),
                ("src4", ctypes.c_uint8), ("word4", ctypes.c_uint8), ("result", ctypes.c_uint8), ("next", ctypes.c_uint8),
                ("act_first", ctypes.c_uint16), ("act_count", ctypes.c_uint16),
                ("k1", ctypes.c_int64), ("k2", ctypes.c_int64), ("k3", ctypes.c_int64), ("k4", ctypes.c_int64)]


class AgxAct(ctypes.Structure):
    """include/akka_gpu.h agx_act (32 B)."""
    _fields_ = [("op", ctypes.c_uint8), ("word", ctypes.c_uint8), ("src", ctypes.c_uint8), ("sword", ctypes.c_uint8),
                ("dsrc", ctypes.c_uint8), ("dword", ctypes.c_uint8), ("pad0", ctypes.c_uint8), ("pad1", ctypes.c_uint8),
                ("or_mask", ctypes.c_uint32), ("k", ctypes.c_int64), ("dk", ctypes.c_int64)]


class AgxSupervisor(ctypes.Structure):
    """include/akka_gpu.h agx_supervisor (32 B)."""
    _fields_ = [("class_mask", ctypes.c_uint32), ("strategy", ctypes.c_uint8), ("reset_mask", ctypes.c_uint8),
                ("pad0", ctypes.c_uint8), ("pad1", ctypes.c_uint8), ("max_restarts", ctypes.c_int32),
                ("within", ctypes.c_uint32), ("reset", ctypes.c_uint64 * 2)]


class AgxBackoff(ctypes.Structure):
    """include/akka_gpu.h agx_backoff (20 B)."""
    _fields_ = [("min_backoff", ctypes.c_uint32), ("max_backoff", ctypes.c_uint32), ("random_factor_q16", ctypes.c_uint32),
                ("reset_after", ctypes.c_uint32), ("stash_capacity", ctypes.c_int32)]


assert ctypes.sizeof(AgxCase) == 48 and ctypes.sizeof(AgxAct) == 32 and ctypes.sizeof(AgxSupervisor) == 32
assert ctypes.sizeof(AgxBackoff) == 20


class CompileError(ValueError):
    """The behaviour uses something the tables cannot express."""


# ------------------------------------------------------------------ symbolic values
@dataclass(frozen=True)
class Operand:
    """value = base(src, word) + k (u64 wrapping)."""
    src: int
    word: int = 0
    k: int = 0

    def __add__(self, c):
        if not isinstance(c, int):
            raise CompileError("only a constant can be added to an operand")
        return Operand(self.src, self.word, self.k + c)

    def __sub__(self, c):
        return self + (-c)

    def _test(self, cmp, other):
        return Test(cmp, self, lift(other))

    def __eq__(self, o):  # noqa: D105 -- builds a Test, like the Scala `==` inside a guard
        return self._test(CMP_EQ, o)

    def __ne__(self, o):
        return self._test(CMP_NE, o)

    def __lt__(self, o):
        return self._test(CMP_LT, o)

    def __le__(self, o):
        return self._test(CMP_LE, o)

    def __gt__(self, o):
        return self._test(CMP_GT, o)

    def __ge__(self, o):
        return self._test(CMP_GE, o)

    __hash__ = object.__hash__


def lift(x) -> Operand:
    if isinstance(x, Operand):
        return x
    if isinstance(x, (int, np.integer)):
        return Operand(V_CONST, 0, int(x))
    raise CompileError(f"not an operand: {x!r}")


@dataclass(frozen=True)
class Test:
    cmp: int
    lhs: Operand
    rhs: Operand


ALWAYS = Test(CMP_ANY, Operand(V_CONST), Operand(V_CONST))


@dataclass(frozen=True)
class Action:
    op: int
    word: int = 0
    val: Operand = Operand(V_CONST)
    dst: Operand | None = None
    or_mask: int = 0
    site: object = None   # A_SPAWN: the _SpawnSite
    into: bool = False    # A_SPAWN: state word `word` receives the child's id
    key: object = None    # A_REGISTER / A_DEREGISTER / A_ROUTE: the ServiceKey
    flags: int = 0        # A_ROUTE / A_TELL: ROUTE_KEEP_SENDER, ROUTE_BY_INDEX (pad0)
    ask: object = None    # A_ASK_ARM: (the target's dst operand, the request's operand, its or_mask, adapt tag or None)
    listing: object = None  # A_SUBSCRIBE_LISTING / A_FIND: the MessageType of the key's Listing
    vnf: int = 0          # A_ROUTE with ROUTE_HASHED: the router's virtualNodesFactor (0: whatever the tables' other routers say)


class Field(Operand):
    """A state field (state word 0 or 1)."""

    def set(self, v):
        return Action(A_SET, self.word, lift(v))

    def add(self, v):
        return Action(A_ADD, self.word, lift(v))

    def inc(self, n: int = 1):
        return self.add(n)

    def max(self, v):
        return Action(A_MAX, self.word, lift(v))

    def min(self, v):
        return Action(A_MIN, self.word, lift(v))

    @property
    def ref(self) -> "Ref":
        """The field's value as an ActorRef (an actor id)."""
        return Ref(Operand(V_WORD, self.word))


@dataclass(frozen=True)
class Ref:
    """An ActorRef: `dst` operand; based on the actor's own id it wraps mod n (ring neighbours)."""
    dst: Operand

    def tell(self, msg, tag: int | None = None):
        """ActorRef.! (AA/ActorRef.scala:412-413).  `msg`: an operand (the payload) or a
        MessageType application; `tag` ORs a message tag into the payload."""
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        if tag is not None:
            mask |= (tag & 0xFF) << 24
        return Action(A_TELL, 0, val, self.dst, mask)

    __call__ = tell

    def forward(self, msg, tag: int | None = None):
        """ref.forward(msg): a tell that keeps the incoming message's sender on the envelope (the typed message's
        replyTo travels on).  The actors need an engine with the receptionist (engine.set_receptionist)."""
        a = self.tell(msg, tag)
        return Action(a.op, a.word, a.val, a.dst, a.or_mask, flags=ROUTE_KEEP_SENDER)


def self_ref(offset: int = 0) -> Ref:
    """context.self, or the actor `offset` ids further on (mod the population)."""
    return Ref(Operand(V_SELF, 0, offset))


def actor_ref(actor_id: int) -> Ref:
    return Ref(Operand(V_CONST, 0, actor_id))


@dataclass(frozen=True)
class Message:
    """An outgoing message of a MessageType: payload = (tag << 24) | arg."""
    arg: Operand
    or_mask: int


@dataclass(frozen=True)
class MessageType:
    """A message class: its instances are the payloads carrying `tag` in bits 24..31."""
    name: str
    tag: int

    def __post_init__(self):
        if not 0 <= self.tag <= 0xFF:
            raise CompileError("message tags are 8 bits")

    def __call__(self, arg=0) -> Message:
        return Message(lift(arg), self.tag << 24)

    def payload(self, arg: int = 0) -> int:
        """The u32 payload of an instance (for host tells)."""
        return (self.tag << 24) | (arg & 0xFFFFFF)


@dataclass(frozen=True)
class ServiceKey:
    """ServiceKey[T](id) (TY/receptionist/Receptionist.scala): names a service; keys with the same name are the
    same key.  The lowering numbers the keys in use, at most MAX_SERVICE_KEYS, in order of first appearance."""
    name: str


@dataclass(frozen=True)
class EntityTypeKey:
    """EntityTypeKey[T](name) (akka-cluster-sharding-typed EntityTypeKey): names an entity type."""
    name: str


class _EntityId:
    def __repr__(self):
        return "Entity.ID"


class Entity:
    """Entity(typeKey)(createBehavior) (akka-cluster-sharding-typed Entity): the ids [first_id, first_id + count) are
    the type's entities.  They are not registered: an entity starts in `behavior` on its first message with state word
    0 = `word0` and word 1 = `word1` (a constant, or Entity.ID: the entity's id).  ``with_stop_message(msg)`` is the
    message context.passivate() makes the shard send (required); ``with_receive_timeout(delay, msg)`` sets the
    receive timeout of every start."""
    ID = _EntityId()

    def __init__(self, key, behavior, first_id: int, count: int, word0: int = 0, word1=0):
        if not isinstance(key, EntityTypeKey):
            raise CompileError(f"Entity takes an EntityTypeKey, not {key!r}")
        if not isinstance(behavior, Behavior):
            raise CompileError(f"Entity takes a Behavior, not {behavior!r}")
        if not isinstance(first_id, (int, np.integer)) or not isinstance(count, (int, np.integer)) or first_id < 0 or count < 1:
            raise CompileError(f"an entity range is [first_id, first_id + count) with count >= 1, not ({first_id!r}, {count!r})")
        if not isinstance(word0, (int, np.integer)) or not 0 <= int(word0) < (1 << 64):
            raise CompileError(f"an entity's word 0 is a u64 constant, not {word0!r}")
        if word1 is not self.ID and (not isinstance(word1, (int, np.integer)) or not 0 <= int(word1) < (1 << 64)):
            raise CompileError(f"an entity's word 1 is a u64 constant or Entity.ID, not {word1!r}")
        self.key, self.behavior, self.first_id, self.count = key, behavior, int(first_id), int(count)
        self.word0, self.word1 = int(word0), None if word1 is self.ID else int(word1)
        self.stop_payload = None
        self.idle = (0, 0)

    @staticmethod
    def _payload(msg, what) -> int:
        if isinstance(msg, Message):
            if msg.arg.src != V_CONST:
                raise CompileError(f"{what} is a constant message")
            return ((msg.arg.k & 0xFFFFFF) | msg.or_mask) & 0xFFFFFFFF
        if isinstance(msg, (int, np.integer)):
            return int(msg) & 0xFFFFFFFF
        raise CompileError(f"{what} is a MessageType application or a u32 payload, not {msg!r}")

    def with_stop_message(self, msg) -> "Entity":
        self.stop_payload = self._payload(msg, "an entity's stop message")
        return self

    def with_receive_timeout(self, delay: int, msg) -> "Entity":
        if not isinstance(delay, (int, np.integer)) or not 1 <= int(delay) <= MAX_TIMER_DELAY:
            raise CompileError(f"an entity's receive timeout is 1..{MAX_TIMER_DELAY} ticks, not {delay!r}")
        self.idle = (int(delay), self._payload(msg, "an entity's receive-timeout message"))
        return self


@dataclass(frozen=True)
class Topic:
    """Topic[T](name) (TY/pubsub/Topic.scala; TopicImpl.scala:60-143): names a pub-sub topic; topics with the same
    name are the same topic.  A topic is a service key of its own (the reference's topicServiceKey): the lowering
    numbers topics and ServiceKeys together, at most MAX_SERVICE_KEYS of both, in order of first appearance."""
    name: str


@dataclass(frozen=True)
class _KeyOperand(Operand):
    """An operand that reads a key's listing: `word` is filled in by the lowering (key index | selector << 3)."""
    key: ServiceKey | None = None
    sel: int = 0

    def __add__(self, c):
        if not isinstance(c, int):
            raise CompileError("only a constant can be added to an operand")
        return _KeyOperand(self.src, self.word, self.k + c, self.key, self.sel)

    __eq__ = Operand.__eq__
    __hash__ = object.__hash__


class Incoming:
    """The message being handled (symbolic)."""
    payload = Operand(V_PAYLOAD)
    tag = Operand(V_TAG)
    arg = Operand(V_ARG)
    sender = Ref(Operand(V_SENDER))


class State:
    """Named state fields -> words 0, 1."""

    def __init__(self, *names: str):
        if len(names) > 2:
            raise CompileError("compiled behaviours hold at most two u64 state fields")
        self.names = names
        for i, n in enumerate(names):
            setattr(self, n, Field(V_WORD, i))


# ------------------------------------------------------------------ behaviours
@dataclass(frozen=True)
class _Result:
    code: int
    name: str


@dataclass(frozen=True, eq=False)
class _StashEffect:
    """buffer.stash(msg): the last effect of a case (the message is kept, the behaviour stays)."""
    buffer: "StashBuffer"


@dataclass(frozen=True, eq=False)
class _UnstashAll:
    """buffer.unstashAll(behavior) as a case's result."""
    buffer: "StashBuffer"
    target: object  # Behavior or Behaviors.same


class StashBuffer:
    """StashBuffer[T] (TY/scaladsl/StashBuffer.scala; StashBufferImpl.scala:61-79 stash / capacity,
    :131-218 unstashAll) of the actor running the behaviour, symbolic.  The engine enforces the stash
    capacity of the actor's mailbox class (engine.set_stash), not this number: `capacity` only feeds
    `is_full` and Tables.stash_capacity, so bind such behaviours to a class with the same capacity wherever
    a case tests `is_full` (a smaller class capacity overflows earlier than `is_full` says)."""

    def __init__(self, capacity: int):
        if not isinstance(capacity, int) or not 1 <= capacity <= MAX_STASH:
            raise CompileError(f"a stash holds 1..{MAX_STASH} messages (no unbounded stash), not {capacity!r}")
        self.capacity = capacity
        self.size = Operand(V_STASH)

    def stash(self) -> _StashEffect:
        return _StashEffect(self)

    def unstash_all(self, behavior) -> _UnstashAll:
        if not (isinstance(behavior, Behavior) or behavior is Behaviors.same):
            raise CompileError("unstash_all takes a Behavior or Behaviors.same")
        return _UnstashAll(self, behavior)

    @property
    def is_empty(self) -> Test:
        return self.size == 0

    @property
    def non_empty(self) -> Test:
        return self.size > 0

    @property
    def is_full(self) -> Test:
        return self.size >= self.capacity


class TimerScheduler:
    """TimerScheduler[T] (TY/scaladsl/TimerScheduler.scala; TY/internal/TimerSchedulerImpl.scala:61-172) of the
    actor running the behaviour, symbolic.  Time is logical: a delay is a count of ticks (supersteps), at least 1.
    The scheduled task is only `self ! timerMsg`, so start_timer_with_fixed_delay and start_timer_at_fixed_rate
    coincide (both fire at start + d, start + 2d, ...) and lower to one periodic action.  Keys are mapped to the
    actor's timer slots 0..3 in the order they first appear.  A start used as an effect of a handler runs when
    the message is handled; a start made in the with_timers block itself and not used as an effect is a setup
    start: it is recorded (Tables.initial_timers) and needs a constant delay and message."""

    def __init__(self):
        self.keys: dict = {}
        self._starts: list = []  # every start action created, in order

    def _key(self, key) -> int:
        if key not in self.keys:
            if len(self.keys) >= MAX_TIMER_KEYS:
                raise CompileError(f"an actor has at most {MAX_TIMER_KEYS} timer keys")
            self.keys[key] = len(self.keys)
        return self.keys[key]

    def _start(self, op, key, msg, delay) -> "Action":
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        d = lift(delay)
        if d.src == V_CONST and d.k < 1:
            raise CompileError(f"a timer delay is at least 1 tick, not {d.k}")
        if d.src == V_CONST and d.k > MAX_TIMER_DELAY:
            raise CompileError(f"a timer delay is at most {MAX_TIMER_DELAY} ticks")
        a = Action(op, self._key(key), val, d, mask)
        self._starts.append(a)
        return a

    def start_single_timer(self, key, msg, delay) -> "Action":
        """startSingleTimer(key, msg, delay)."""
        return self._start(A_TIMER_SINGLE, key, msg, delay)

    def start_timer_with_fixed_delay(self, key, msg, delay) -> "Action":
        """startTimerWithFixedDelay(key, msg, delay): periodic (the same op as start_timer_at_fixed_rate)."""
        return self._start(A_TIMER_PERIODIC, key, msg, delay)

    def start_timer_at_fixed_rate(self, key, msg, interval) -> "Action":
        """startTimerAtFixedRate(key, msg, interval): periodic (the same op as start_timer_with_fixed_delay)."""
        return self._start(A_TIMER_PERIODIC, key, msg, interval)

    def cancel(self, key) -> "Action":
        return Action(A_TIMER_CANCEL, self._key(key))

    def cancel_all(self) -> "Action":
        return Action(A_TIMER_CANCEL_ALL, 0)

    def is_timer_active(self, key) -> Test:
        """isTimerActive(key) as a test."""
        return Operand(V_TIMER, self._key(key)) == 1


_TIMER_SCOPES: list = []  # the TimerSchedulers of the with_timers blocks being built, innermost last (context.ask)


class _Parent:
    """context.PARENT: a spawned child's state word 1 starts as its parent's id."""

    def __repr__(self):
        return "context.PARENT"


@dataclass(frozen=True, eq=False)
class _SpawnSite:
    """What a child starts as: its behaviour, the base of state word 0, state word 1 (None: the parent's id)."""
    behavior: "Behavior"
    base: int
    word1: int | None


class ActorContext:
    """ActorContext[T]'s death watch (TY/scaladsl/ActorContext.scala watch / watchWith / unwatch; classic
    AA/dungeon/DeathWatch.scala:19-113) of the actor running the behaviour, symbolic: the calls return effects.
    The actors need an engine with death watch (engine.set_death_watch); an actor watches at most
    MAX_WATCH_SLOTS refs at a time, and host-side actors cannot be watched."""

    @staticmethod
    def _ref(ref) -> Operand:
        if not isinstance(ref, Ref):
            raise CompileError(f"not an ActorRef: {ref!r}")
        return ref.dst

    def watch(self, ref) -> "Action":
        """context.watch(ref): Terminated(ref) arrives as a signal once `ref` has stopped (on_signal); a behaviour
        without a matching signal case fails with the death pact."""
        return Action(A_WATCH, 0, Operand(V_CONST), self._ref(ref), 0)

    def watch_with(self, ref, msg) -> "Action":
        """context.watchWith(ref, msg): `msg` arrives as an ordinary message, its sender the terminated ref."""
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        return Action(A_WATCH_WITH, 0, val, self._ref(ref), mask)

    def unwatch(self, ref) -> "Action":
        """context.unwatch(ref): a Terminated of it that is already enqueued is dropped at receipt."""
        return Action(A_UNWATCH, 0, Operand(V_CONST), self._ref(ref), 0)

    # children (engine.set_children(regions, tables.spawn_sites); TY/scaladsl/ActorContext.scala spawnAnonymous / stop)
    PARENT = _Parent()

    def spawn(self, behavior, arg=0, word1=0, into=None, base: int = 0) -> "Action":
        """context.spawn(behavior): the actor's next child starts in `behavior` with state word 0 = base + arg (the
        low 18 bits of `arg`, an operand) and state word 1 = `word1` (a constant, or context.PARENT: the parent's
        id).  `into`: a state field of the parent that receives the child's id (0xFFFFFFFF when the spawn is
        refused: the actor lies in no parent range or its child block is full).  The child's id is fixed by the
        engine's regions.  A case holds at most one of tell, spawn and stop."""
        if not isinstance(behavior, Behavior):
            raise CompileError(f"spawn takes a Behavior, not {behavior!r}")
        if word1 is not self.PARENT and (not isinstance(word1, (int, np.integer)) or not 0 <= int(word1) < (1 << 64)):
            raise CompileError(f"a child's word 1 is a u64 constant or context.PARENT, not {word1!r}")
        if not isinstance(base, (int, np.integer)) or not 0 <= int(base) < (1 << 64):
            raise CompileError(f"a spawn site's base is a u64 constant, not {base!r}")
        if into is not None and not isinstance(into, Field):
            raise CompileError(f"into= names a state field of the parent, not {into!r}")
        a = lift(arg)
        if a.src == V_CONST and not 0 <= a.k < (1 << SPAWN_ARG_BITS):
            raise CompileError(f"a spawn argument has {SPAWN_ARG_BITS} bits: {a.k} does not fit")
        return Action(A_SPAWN, into.word if into is not None else 0, a, None, 0,
                      _SpawnSite(behavior, int(base), None if word1 is self.PARENT else int(word1)), into is not None)

    def stop(self, ref) -> "Action":
        """context.stop(child): the child stops at the start of the next tick.  A ref that is not one of the actor's
        spawned children (the actor itself included) is the reference's IllegalArgumentException: the actor stops."""
        return Action(A_STOP_CHILD, 0, Operand(V_CONST), self._ref(ref), 0)

    def child_at(self, x) -> Ref:
        """The actor's child number x mod its spawn count (x: a state field, + a constant, or a constant) -- the
        routee of a round-robin pool; 0xFFFFFFFF (a dead letter) without children."""
        if isinstance(x, Operand) and x.src == V_WORD:
            return Ref(Operand(V_CHILD, x.word, x.k))
        if isinstance(x, (int, np.integer)):
            return Ref(Operand(V_CHILD, CHILD_NO_WORD, int(x)))
        raise CompileError(f"child_at takes a state field or a constant, not {x!r}")

    @property
    def spawned(self) -> Operand:
        """The number of children the actor has spawned so far."""
        return Operand(V_SPAWNED)

    # receive timeouts (engine.set_receive_timeout on top of engine.set_timers; AA/dungeon/ReceiveTimeout.scala:18-74,
    # typed TY/internal/adapter/ActorContextAdapter.scala:120-131)
    def set_receive_timeout(self, delay, msg) -> "Action":
        """context.setReceiveTimeout(delay, msg): `msg` arrives, its sender the actor itself, once the actor has
        processed no influencing message for `delay` ticks (an operand or a constant of at least 1), and again
        every `delay` ticks while it stays idle.  Messages of the types named in
        compile_behaviors(transparent=...) do not push the timeout back."""
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        d = lift(delay)
        if d.src == V_CONST and d.k < 1:
            raise CompileError(f"a receive timeout is at least 1 tick, not {d.k}")
        if d.src == V_CONST and d.k > MAX_TIMER_DELAY:
            raise CompileError(f"a receive timeout is at most {MAX_TIMER_DELAY} ticks")
        return Action(A_SET_RECEIVE_TIMEOUT, 0, val, d, mask)

    def cancel_receive_timeout(self) -> "Action":
        """context.cancelReceiveTimeout(): an envelope already enqueued stays in the mailbox and is discarded."""
        return Action(A_CANCEL_RECEIVE_TIMEOUT, 0)

    # sharded entities (engine.set_sharding on top of engine.set_receive_timeout; akka-cluster-sharding Shard.scala:405-417)
    def passivate(self) -> "Action":
        """context.parent ! Passivate(stopMessage): the shard marks the entity as passivating and sends it its type's
        stop message; what arrives behind that message is buffered and starts the entity again.  It is the case's one
        envelope.  Run by an actor that is no entity it does nothing (counted)."""
        return Action(A_PASSIVATE, 0)

    # the ask pattern (engine.set_ask on top of engine.set_timers; TY/internal/ActorContextImpl.scala:203-218,
    # TY/scaladsl/AskPattern.scala:109-162)
    @staticmethod
    def _scheduler() -> "TimerScheduler":
        if not _TIMER_SCOPES:
            raise CompileError("context.ask lives inside Behaviors.with_timers: an ask takes one of the actor's timer keys")
        return _TIMER_SCOPES[-1]

    def ask(self, ref, msg, timeout, on_timeout, on_success=None, key=None) -> "Action":
        """context.ask(ref, createRequest)(mapResponse)(timeout): `msg` goes to `ref` with an ask ref as its sender
        (the typed message's replyTo); whatever is told to that ref within `timeout` ticks (an operand or a constant
        of at least 1; a round trip takes 2) comes back with the actor itself as the sender and, with `on_success` (a
        MessageType), that type's tag over its argument; otherwise `on_timeout` arrives.  A later reply is dropped.
        The ask takes a timer key: `key`, or one of its own per ask site; asking again on a key supersedes the
        earlier ask.  It is the case's one envelope."""
        ts = self._scheduler()
        req, req_mask = (msg.arg, msg.or_mask) if isinstance(msg, Message) else (lift(msg), 0)
        val, mask = (on_timeout.arg, on_timeout.or_mask) if isinstance(on_timeout, Message) else (lift(on_timeout), 0)
        if on_success is not None and not isinstance(on_success, MessageType):
            raise CompileError(f"on_success= takes a MessageType or None, not {on_success!r}")
        d = lift(timeout)
        if d.src == V_CONST and d.k < 1:
            raise CompileError(f"an ask's timeout is at least 1 tick, not {d.k}")
        if d.src == V_CONST and d.k > MAX_TIMER_DELAY:
            raise CompileError(f"an ask's timeout is at most {MAX_TIMER_DELAY} ticks")
        if key is None:
            key = ("ask site", len(ts.keys), object())
        if key not in ts.keys and len(ts.keys) >= MAX_TIMER_KEYS:
            raise CompileError(f"an ask takes a timer key and an actor has at most {MAX_TIMER_KEYS}: this ask would be key "
                               f"{len(ts.keys) + 1}")
        return Action(A_ASK_ARM, ts._key(key), val, d, mask,
                      ask=(self._ref(ref), req, req_mask, None if on_success is None else on_success.tag))

    def ask_pending(self, key) -> Test:
        """Is the ask made with key=`key` still outstanding (neither answered, timed out nor cancelled)?"""
        return Operand(V_TIMER, self._scheduler()._key(key)) == 1

    # the receptionist and group routers (engine.set_receptionist(len(tables.service_keys), capacity); TY/internal/
    # receptionist/LocalReceptionist.scala:147-248, TY/internal/routing/GroupRouterImpl.scala:114-146)
    @staticmethod
    def _key(key) -> ServiceKey:
        if not isinstance(key, ServiceKey):
            raise CompileError(f"not a ServiceKey: {key!r}")
        return key

    def register(self, key) -> "Action":
        """context.system.receptionist ! Receptionist.Register(key, context.self): the actor is in the key's listing
        from the next tick on.  Idempotent; an actor only registers itself; no Registered acknowledgement."""
        return Action(A_REGISTER, 0, key=self._key(key))

    def deregister(self, key) -> "Action":
        """receptionist ! Receptionist.Deregister(key, context.self): the actor leaves the listing from the next tick on."""
        return Action(A_DEREGISTER, 0, key=self._key(key))

    def listing_size(self, key) -> Operand:
        """The size of the key's listing in force this tick (Receptionist.Find, read synchronously)."""
        return _KeyOperand(V_LISTING_SIZE, 0, 0, self._key(key), 0)

    def service_at(self, key, x) -> Ref:
        """listing[x mod size] of the key's listing in force (x: a state field, the message's argument, each + a
        constant, or a constant); 0xFFFFFFFF (a dead letter) when the listing is empty."""
        key = self._key(key)
        if isinstance(x, (int, np.integer)):
            return Ref(_KeyOperand(V_SERVICE_AT, 0, int(x), key, SVC_CONST))
        if isinstance(x, Operand) and x.src == V_WORD:
            return Ref(_KeyOperand(V_SERVICE_AT, 0, x.k, key, SVC_WORD0 + x.word))
        if isinstance(x, Operand) and x.src == V_ARG:
            return Ref(_KeyOperand(V_SERVICE_AT, 0, x.k, key, SVC_ARG))
        raise CompileError(f"service_at takes a state field, the message's argument or a constant, not {x!r}")

    def _route(self, key, msg, word, dst, flags) -> "Action":
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        return Action(A_ROUTE, word, val, dst, mask, key=self._key(key), flags=flags)

    def route(self, key, msg, cursor, forward: bool = True) -> "Action":
        """Round-robin routing over the key's listing in force: the routee is the smallest listed id >= the cursor
        (a state field of the router), else listing[0]; the cursor becomes routee + 1.  An empty listing sends the
        message to deadLetters (the reference's Dropped) and leaves the cursor.  `forward`: the envelope keeps the
        incoming message's sender (a typed router passes the message, replyTo included, unchanged)."""
        if not isinstance(cursor, Field):
            raise CompileError(f"cursor= names a state field of the router, not {cursor!r}")
        return self._route(key, msg, cursor.word, None, ROUTE_KEEP_SENDER if forward else 0)

    def route_by(self, key, index, msg, forward: bool = True) -> "Action":
        """Routing by index: the routee is listing[index mod size] -- the same index reaches the same routee while the
        listing stands (the modulo stand-in for consistent hashing)."""
        return self._route(key, msg, 0, lift(index), ROUTE_BY_INDEX | (ROUTE_KEEP_SENDER if forward else 0))

    # consistent-hashing and random routing (engine.set_router_logics after engine.set_receptionist; TY/internal/
    # routing/RoutingLogic.scala:77-112)
    def route_hashed(self, key, hash_key, msg, forward: bool = True, virtual_nodes_factor: int = 0) -> "Action":
        """Consistent-hashing routing: the routee is nodeFor(str(hash_key mod 2^32)) on the key's hash ring in force --
        a change of the listing moves only the hash keys of the nodes that came or went.  An empty ring is an empty
        listing."""
        if isinstance(virtual_nodes_factor, bool) or not isinstance(virtual_nodes_factor, (int, np.integer)) or virtual_nodes_factor < 0:
            raise CompileError("virtualNodesFactor has to be a positive integer")
        if virtual_nodes_factor > MAX_VIRTUAL_NODES:
            raise CompileError(f"virtualNodesFactor is at most {MAX_VIRTUAL_NODES}, not {virtual_nodes_factor}")
        a = self._route(key, msg, 0, lift(hash_key), ROUTE_HASHED | (ROUTE_KEEP_SENDER if forward else 0))
        return Action(a.op, a.word, a.val, a.dst, a.or_mask, key=a.key, flags=a.flags, vnf=int(virtual_nodes_factor))

    def route_random(self, key, msg, counter, forward: bool = True) -> "Action":
        """Random routing: the routee is listing[r mod size], r drawn from the engine's seed, the router's id and the
        counter (a state field of the router), which then grows by one; it stays when there is no routee."""
        if not isinstance(counter, Field):
            raise CompileError(f"counter= names a state field of the router, not {counter!r}")
        return self._route(key, msg, counter.word, None, ROUTE_RANDOM | (ROUTE_KEEP_SENDER if forward else 0))

    # Subscribe / Find and the Listing message (engine.set_listings after engine.set_topics; TY/internal/receptionist/
    # LocalReceptionist.scala:152-171,209-220)
    def _listing(self, op: int, key, listing_msg) -> "Action":
        if isinstance(key, Topic):
            raise CompileError(f"a Topic has no Listing: subscribe to it with context.subscribe ({key!r})")
        if not isinstance(listing_msg, MessageType):
            raise CompileError(f"the Listing of a key is a MessageType: {listing_msg!r}")
        return Action(op, 0, key=self._key(key), listing=listing_msg)

    def receptionist_subscribe(self, key, listing_msg) -> "Action":
        """receptionist ! Receptionist.Subscribe(key, context.self): the actor receives `listing_msg(key number)` in
        the next tick (the current listing, on every Subscribe) and after every tick in which the key's listing
        changed, until it stops; the handler reads the set with context.listing_size(key) / service_at(key, x).  Not
        an envelope of the case."""
        return self._listing(A_SUBSCRIBE_LISTING, key, listing_msg)

    def receptionist_find(self, key, listing_msg) -> "Action":
        """receptionist ! Receptionist.Find(key, context.self): one `listing_msg(key number)` in the next tick."""
        return self._listing(A_FIND, key, listing_msg)

    # pub-sub topics (engine.set_topics after engine.set_receptionist; TY/internal/pubsub/TopicImpl.scala:60-143)
    @staticmethod
    def _topic(topic) -> Topic:
        if not isinstance(topic, Topic):
            raise CompileError(f"not a Topic: {topic!r}")
        return topic

    def subscribe(self, topic) -> "Action":
        """topic ! Topic.Subscribe(context.self): the actor receives what is published from this tick on (a
        publication of this very tick included).  Idempotent; a stop unsubscribes."""
        return Action(A_REGISTER, 0, key=self._topic(topic))

    def unsubscribe(self, topic) -> "Action":
        """topic ! Topic.Unsubscribe(context.self): the publications of this tick no longer reach the actor."""
        return Action(A_DEREGISTER, 0, key=self._topic(topic))

    def publish(self, topic, msg) -> "Action":
        """topic ! Topic.Publish(msg): every subscriber receives `msg` in the next tick, with this actor as its
        sender.  It is the case's one envelope: a case holds at most one of tell, route and publish."""
        if isinstance(msg, Message):
            val, mask = msg.arg, msg.or_mask
        else:
            val, mask = lift(msg), 0
        return Action(A_PUBLISH, 0, val, None, mask, key=self._topic(topic))

    def subscriber_count(self, topic) -> Operand:
        """The topic's subscribers as of the end of the tick before (Topic.GetTopicStats, read synchronously)."""
        return _KeyOperand(V_LISTING_SIZE, 0, 0, self._topic(topic), 0)


context = ActorContext()


class _GroupRouter:
    """Routers.group(key) (TY/scaladsl/Routers.scala; GroupRouterImpl.scala:114-146): the builder."""

    def __init__(self, key):
        self.key, self.index = ActorContext._key(key), None
        self.logic, self.vnf = "round_robin", 0

    def with_round_robin_routing(self) -> "_GroupRouter":
        """withRoundRobinRouting (RoutingLogic.scala:42-75): the default here."""
        self.index, self.logic = None, "round_robin"
        return self

    def with_index_routing(self, index) -> "_GroupRouter":
        """Routing by `index(m)` mod the listing's size, e.g. lambda m: m.arg."""
        self.index, self.logic = index, "index"
        return self

    def with_random_routing(self) -> "_GroupRouter":
        """withRandomRouting (RoutingLogic.scala:77-91): a counter-based draw per message (word 0 of the router)."""
        self.index, self.logic = None, "random"
        return self

    def with_consistent_hash_routing(self, virtual_nodes_factor: int, mapping) -> "_GroupRouter":
        """withConsistentHashingRouting(virtualNodesFactor, mapping) (RoutingLogic.scala:93-112): `mapping(m)` is the
        operand whose low 32 bits, as a decimal string, are the message's hash key, e.g. lambda m: m.arg."""
        if isinstance(virtual_nodes_factor, bool) or not isinstance(virtual_nodes_factor, (int, np.integer)) or virtual_nodes_factor < 1:
            raise CompileError("virtualNodesFactor has to be a positive integer")
        self.index, self.logic, self.vnf = mapping, "hashed", int(virtual_nodes_factor)
        return self

    def build(self, name: str = "group_router") -> "Behavior":
        """The router as a Behavior over State("cursor", "routed"): every message is forwarded, payload unchanged,
        to the routee the logic selects; `routed` counts the messages seen."""
        st = State("cursor", "routed")
        if self.logic == "random":
            h = lambda m, s: [s.routed.inc(), context.route_random(self.key, m.payload, counter=s.cursor), Behaviors.same]
        elif self.logic == "hashed":
            h = lambda m, s: [s.routed.inc(), context.route_hashed(self.key, self.index(m), m.payload,
                                                                   virtual_nodes_factor=self.vnf), Behaviors.same]
        elif self.index is None:
            h = lambda m, s: [s.routed.inc(), context.route(self.key, m.payload, cursor=s.cursor), Behaviors.same]
        else:
            h = lambda m, s: [s.routed.inc(), context.route_by(self.key, self.index(m), m.payload), Behaviors.same]
        return ReceiveBuilder.create(st).on_any_message(h).build(name)


class Routers:
    """Routers.group(key): a group router over the actors registered under `key` (pool routers: workloads.pool_router)."""

    @staticmethod
    def group(key) -> _GroupRouter:
        return _GroupRouter(key)


class Terminated:
    """The Terminated signal (TY/MessageAndSignals.scala) as a handler sees it: `sig.ref` is the terminated ref."""
    ref = Ref(Operand(V_SENDER))


class PreRestart:
    """The PreRestart signal (TY/MessageAndSignals.scala): it runs on the failing behaviour before a restart."""
    code = SIGNAL_PRERESTART


class PostStop:
    """The PostStop signal: it runs on the current behaviour at every stop of the actor."""
    code = SIGNAL_POSTSTOP


class ExceptionType:
    """An exception class a handler may throw (Behaviors.throw) and a supervisor may catch (on_failure).  `parent`
    defaults to Throwable, the root; a supervisor of a class catches it and its descendants, so the root catches
    all.  The lowering numbers the classes used (at most 32) and flattens the hierarchy into masks."""

    def __init__(self, name: str, parent: "ExceptionType | None" = None):
        if parent is not None and not isinstance(parent, ExceptionType):
            raise CompileError(f"not an ExceptionType: {parent!r}")
        self.name = name
        self.parent = parent if parent is not None else getattr(ExceptionType, "root", None)

    def is_a(self, other: "ExceptionType") -> bool:
        x = self
        while x is not None:
            if x is other:
                return True
            x = x.parent
        return False

    def __repr__(self):
        return f"ExceptionType({self.name})"


ExceptionType.root = Throwable = ExceptionType("Throwable")


@dataclass(frozen=True, eq=False)
class _Throw:
    """Behaviors.throw(exc) as a case's result."""
    exc: ExceptionType


@dataclass(frozen=True)
class _Strategy:
    """A SupervisorStrategy value (TY/SupervisorStrategy.scala): resume, stop, restart [with a limit]."""
    kind: int
    max_restarts: int = -1
    within: int = 1


class _Restart(_Strategy):
    def with_limit(self, max_restarts: int, within: int) -> _Strategy:
        """restart.withLimit(maxNrOfRetries, withinTimeRange): `within` in ticks (supersteps with mail), >= 1."""
        if not isinstance(max_restarts, int) or max_restarts < 0:
            raise CompileError(f"with_limit: max_restarts is an integer >= 0, not {max_restarts!r}")
        if not isinstance(within, int) or not 1 <= within <= MAX_TIMER_DELAY:
            raise CompileError(f"with_limit: within is a number of ticks >= 1, not {within!r}")
        return _Strategy(SUP_RESTART, max_restarts, within)


@dataclass(frozen=True)
class _Backoff(_Strategy):
    """restartWithBackoff(min, max, randomFactor) (TY/SupervisorStrategy.scala): a restart entry with a backoff row
    (engine.set_backoff(tables.backoff)).  Times are ticks; the defaults are the reference's: no limit, the count
    resets min_backoff after the restart, the stash capacity is the actor's mailbox capacity (-1; the reference's
    configured default is 1000)."""
    min_backoff: int = 1
    max_backoff: int = 1
    random_factor_q16: int = 0
    reset_after: int = 1
    stash_capacity: int = -1

    def with_max_restarts(self, n: int) -> "_Backoff":
        """withMaxRestarts(n): the (n + 1)-th failure stops the actor (-1: no limit)."""
        if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or int(n) < -1 or int(n) > 0x7FFFFFFF:
            raise CompileError(f"with_max_restarts: an integer >= -1, not {n!r}")
        return replace(self, max_restarts=int(n))

    def with_reset_backoff_after(self, ticks: int) -> "_Backoff":
        """withResetBackoffAfter(ticks): the count resets this many ticks after the delayed restart, >= 1."""
        if not isinstance(ticks, (int, np.integer)) or isinstance(ticks, bool) or not 1 <= int(ticks) <= MAX_TIMER_DELAY:
            raise CompileError(f"with_reset_backoff_after: a number of ticks in 1..{MAX_TIMER_DELAY}, not {ticks!r}")
        return replace(self, reset_after=int(ticks))

    def with_stash_capacity(self, n: int) -> "_Backoff":
        """withStashCapacity(n): the messages held while the actor backs off (-1: the mailbox capacity; 0: none)."""
        if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or int(n) < -1 or int(n) > 0x7FFFFFFF:
            raise CompileError(f"with_stash_capacity: an integer >= -1, not {n!r}")
        return replace(self, stash_capacity=int(n))


class SupervisorStrategy:
    """SupervisorStrategy.resume / stop / restart / restart.with_limit(n, within) / restart_with_backoff(min, max,
    random_factor).  Children (stopChildren) and logging are left out."""
    resume = _Strategy(SUP_RESUME)
    stop = _Strategy(SUP_STOP)
    restart = _Restart(SUP_RESTART)

    @staticmethod
    def restart_with_backoff(min_backoff: int, max_backoff: int, random_factor: float) -> _Backoff:
        """restartWithBackoff(minBackoff, maxBackoff, randomFactor): after failure c + 1 the actor restarts and stays
        suspended for min(max_backoff, min_backoff * 2^c) ticks (max_backoff from c = 30 on), plus up to
        random_factor times that as jitter; what arrives meanwhile is held up to the stash capacity.  Chain
        with_max_restarts / with_reset_backoff_after / with_stash_capacity."""
        for name, v in (("min_backoff", min_backoff), ("max_backoff", max_backoff)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= MAX_TIMER_DELAY:
                raise CompileError(f"restart_with_backoff: {name} is a number of ticks in 1..{MAX_TIMER_DELAY}, not {v!r}")
        if int(min_backoff) > int(max_backoff):
            raise CompileError(f"restart_with_backoff: min_backoff {min_backoff} exceeds max_backoff {max_backoff}")
        if not isinstance(random_factor, (int, float, np.integer, np.floating)) or isinstance(random_factor, bool) or \
                not 0.0 <= float(random_factor) <= 1.0:
            raise CompileError(f"restart_with_backoff: random_factor lies in 0.0..1.0, not {random_factor!r}")
        return _Backoff(SUP_RESTART, -1, 1, int(min_backoff), int(max_backoff), int(round(float(random_factor) * 65536)),
                        int(min_backoff), -1)


@dataclass(eq=False)
class _Supervisor:
    strategy: _Strategy
    exc: ExceptionType
    reset: dict  # state word -> value


class _Supervise:
    """Behaviors.supervise(behavior): the wrapper waiting for on_failure."""

    def __init__(self, behavior: "Behavior", reset: dict):
        self.behavior, self.reset = behavior, reset

    def on_failure(self, strategy, exc: ExceptionType | None = None) -> "Behavior":
        """onFailure[exc](strategy): returns the behaviour, supervised; supervise it again for an outer supervisor."""
        if not isinstance(strategy, _Strategy):
            raise CompileError(f"not a SupervisorStrategy: {strategy!r}")
        exc = Throwable if exc is None else exc
        if not isinstance(exc, ExceptionType):
            raise CompileError(f"not an ExceptionType: {exc!r}")
        if len(self.behavior.supervisors) >= MAX_SUPERVISORS:
            raise CompileError(f"a behaviour has at most {MAX_SUPERVISORS} nested supervisors")
        self.behavior.supervisors.append(_Supervisor(strategy, exc, self.reset))
        return self.behavior


class Behaviors:
    """Behaviors.same / stopped / unhandled (TY/scaladsl/Behaviors.scala), receiveMessage, withStash, withTimers,
    supervise and throw."""
    same = _Result(RES_SAME, "same")
    stopped = _Result(RES_STOPPED, "stopped")
    unhandled = _Result(RES_UNHANDLED, "unhandled")

    @staticmethod
    def throw(exc: ExceptionType) -> _Throw:
        """`throw new Exc` as a case's result: the case's effects are those before the throw; the actors need an
        engine with supervision (engine.set_supervision(tables.supervisors))."""
        if not isinstance(exc, ExceptionType):
            raise CompileError(f"not an ExceptionType: {exc!r}")
        return _Throw(exc)

    @staticmethod
    def supervise(behavior: "Behavior", reset: dict | None = None) -> _Supervise:
        """Behaviors.supervise(behavior).on_failure(strategy, exc=...) (TY/internal/Supervision.scala:43-52),
        nestable (the first is the innermost).  `reset`: {field: value} -- the state a restart re-creates; the
        other fields model constructor arguments and stay.  Only an actor's initial behaviour can be supervised."""
        if not isinstance(behavior, Behavior):
            raise CompileError("supervise takes a Behavior")
        words = {}
        for f, v in (reset or {}).items():
            if isinstance(f, str):
                f = getattr(behavior.state, f, None)
            if not isinstance(f, Field):
                raise CompileError("reset maps state fields to values")
            if not isinstance(v, (int, np.integer)) or not 0 <= int(v) < (1 << 64):
                raise CompileError(f"a reset value is a u64 constant, not {v!r}")
            words[f.word] = int(v)
        return _Supervise(behavior, words)

    @staticmethod
    def with_stash(capacity: int, factory) -> "Behavior":
        """Behaviors.withStash(capacity)(factory): `factory(buffer)` builds the behaviour(s) around one
        StashBuffer; the actors running it need a mailbox class with a stash of at least `capacity`."""
        b = factory(StashBuffer(capacity))
        if not isinstance(b, Behavior):
            raise CompileError("with_stash's factory must return a Behavior")
        return b

    @staticmethod
    def with_timers(factory) -> "Behavior":
        """Behaviors.withTimers(factory): `factory(timers)` builds the behaviour(s) around one TimerScheduler.
        Starts made in the block that no handler uses as an effect are the setup starts of the actors that
        begin in the returned behaviour (Tables.initial_timers; engine.start_timers applies them)."""
        ts = TimerScheduler()
        _TIMER_SCOPES.append(ts)
        try:
            b = factory(ts)
        finally:
            _TIMER_SCOPES.pop()
        if not isinstance(b, Behavior):
            raise CompileError("with_timers' factory must return a Behavior")
        used = {id(e) for x in _reachable([b]) for c in x.cases for e in c.effects}
        initial = []
        for a in ts._starts:
            if id(a) in used:
                continue
            if a.val.src != V_CONST or a.dst.src != V_CONST:
                raise CompileError("a timer started in the with_timers block needs a constant delay and message")
            pay = ((a.val.k & 0xFFFFFF) | a.or_mask) if a.or_mask else (a.val.k & 0xFFFFFFFF)
            initial.append((a.word, a.op == A_TIMER_PERIODIC, a.dst.k, pay))
        for x in _reachable([b]):
            if x.timers is None:
                x.timers = ts
        b.initial_timers = initial
        return b

    @staticmethod
    def receive_signal(behavior: "Behavior", handler, when=None, signal=None) -> "Behavior":
        """behavior.receiveSignal { case (_, Terminated(ref)) => ... }: `handler(sig, state)` is appended to
        `behavior` as a signal case of `signal` (Terminated unless given; PreRestart, PostStop) -- the rules are
        ReceiveBuilder.on_signal's; returns `behavior`."""
        rb = ReceiveBuilder.create(behavior.state).on_signal(Terminated if signal is None else signal, handler, when)
        behavior.cases = list(behavior.cases) + rb.cases
        return behavior

    @staticmethod
    def receive_message(state: State, *handlers, name: str = "behavior") -> "Behavior":
        """Behaviors.receiveMessage with a partial function: `handlers` are
        (type or None, handler[, test[, when]]) tuples tried in order."""
        b = ReceiveBuilder.create(state)
        for h in handlers:
            b.on_message(*h)
        return b.build(name)


@dataclass
class _Case:
    tests: list
    effects: list
    result: object  # _Result, Behavior, _StashEffect (stash, then same) or _UnstashAll
    signal: bool = False  # a signal case (on_signal): ordinary messages skip it, signals try only these
    sig_code: int = 0     # SIGNAL_PRERESTART / SIGNAL_POSTSTOP: a supervision signal case (0: Terminated)


@dataclass(eq=False)
class Behavior:
    name: str
    state: State
    cases: list = field(default_factory=list)
    timers: object = None  # the TimerScheduler of the with_timers block the behaviour was built in
    initial_timers: list = field(default_factory=list)  # with_timers' setup starts: (key, periodic, delay, payload)
    supervisors: list = field(default_factory=list)     # Behaviors.supervise(..).on_failure(..), inner first


class ReceiveBuilder:
    """javadsl ReceiveBuilder (TY/javadsl/ReceiveBuilder.scala): handlers in the order added."""

    def __init__(self, state: State):
        self.state = state
        self.cases: list[_Case] = []

    @staticmethod
    def create(state: State | None = None) -> "ReceiveBuilder":
        return ReceiveBuilder(state or State())

    def _add(self, tests, handler, when):
        m, s = Incoming, self.state
        if when is not None:
            tests.append(when(m, s))
        out = handler(m, s)
        if not isinstance(out, (list, tuple)):
            out = [out]
        effects, result = list(out[:-1]), out[-1]
        if isinstance(result, _StashEffect):
            raise CompileError("buffer.stash() is an effect: end the case with Behaviors.same")
        if not isinstance(result, (_Result, Behavior, _UnstashAll, _Throw)):
            raise CompileError("a handler's last element must be Behaviors.same/stopped/unhandled, a Behavior, "
                               "buffer.unstash_all(...) or Behaviors.throw(...)")
        if effects and isinstance(effects[-1], _StashEffect):  # the message is kept: the behaviour stays
            if isinstance(result, _UnstashAll):
                raise CompileError("a case cannot stash its message and unstash_all")
            if result is not Behaviors.same:
                raise CompileError("a case that stashes its message ends with Behaviors.same (not stopped, "
                                   "unhandled or another behaviour)")
            result = effects.pop()
        for e in effects:
            if isinstance(e, _StashEffect):
                raise CompileError("buffer.stash() must be the last effect of a case")
        for e in effects:
            if not isinstance(e, Action):
                raise CompileError(f"not an effect: {e!r}")
        for t in tests:
            if not isinstance(t, Test):
                raise CompileError(f"not a test: {t!r}")
        if len(tests) > 2:
            raise CompileError("a handler has at most two tests (message type / predicate / state guard)")
        self.cases.append(_Case(tests, effects, result))
        return self

    def on_message(self, mtype: MessageType | None, handler, test=None, when=None) -> "ReceiveBuilder":
        """onMessage(type, [test,] handler) (:48-60); `when` guards on the actor's state."""
        tests = [] if mtype is None else [Incoming.tag == mtype.tag]
        if test is not None:
            tests.append(test(Incoming))
        return self._add(tests, handler, when)

    def on_signal(self, signal, handler, when=None) -> "ReceiveBuilder":
        """onSignal(Terminated.class, handler) (:104-122): `handler(sig, state)` sees `sig.ref`, the terminated
        ref; `when` guards on the signal and the state.  Only Terminated is a signal of the compiled subset.  A
        signal case neither stashes nor uses timers."""
        if signal is PreRestart or signal is PostStop:
            # a supervision signal: the first test is payload == the signal (how the engine tells it from Terminated)
            n = len(self.cases)
            self._add([Incoming.payload == signal.code], lambda m, s: handler(signal, s),
                      (lambda m, s: when(signal, s)) if when is not None else None)
            c = self.cases[n]
            if c.result is not Behaviors.same:
                raise CompileError("a PreRestart / PostStop case ends with Behaviors.same (the restart or the stop follows)")
            if any(e.op > A_TELL for e in c.effects) or \
                    any(o.src in (V_TIMER, V_STASH) for t in c.tests for o in (t.lhs, t.rhs)):
                raise CompileError("a PreRestart / PostStop case cannot use timers, death watch or the stash "
                                   "(supervision shares an engine with none of them)")
            c.signal, c.sig_code = True, signal.code
            return self
        if signal is not Terminated:
            raise CompileError("the signals of compiled behaviours are Terminated, PreRestart and PostStop")
        n = len(self.cases)
        self._add([], lambda m, s: handler(Terminated, s), (lambda m, s: when(Terminated, s)) if when is not None else None)
        c = self.cases[n]
        if isinstance(c.result, (_StashEffect, _UnstashAll)):
            raise CompileError("a signal case cannot stash or unstash_all (a signal is no message)")
        if any(A_TIMER_SINGLE <= e.op <= A_TIMER_CANCEL_ALL for e in c.effects) or \
                any(o.src == V_TIMER for t in c.tests for o in (t.lhs, t.rhs)):
            raise CompileError("a signal case cannot use timers (death watch and timers do not share an engine)")
        c.signal = True
        return self

    def on_message_equals(self, payload: int, handler, when=None) -> "ReceiveBuilder":
        """onMessageEquals(msg, handler) (:83-90)."""
        return self._add([Incoming.payload == payload], lambda m, s: handler(m, s), when)

    def on_any_message(self, handler, test=None, when=None) -> "ReceiveBuilder":
        """onAnyMessage(handler) (:98)."""
        return self.on_message(None, handler, test, when)

    def build(self, name: str = "behavior", into: Behavior | None = None) -> Behavior:
        """The built behaviour; `into` fills a Behavior created beforehand (mutually recursive
        behaviours that become each other)."""
        if into is not None:
            into.cases = list(self.cases)
            return into
        return Behavior(name, self.state, list(self.cases))


# ------------------------------------------------------------------ lowering
@dataclass
class Tables:
    """The lowered tables of a set of behaviours (agx_set_behaviors arguments)."""
    behaviors: list
    cases: ctypes.Array
    acts: ctypes.Array
    first: np.ndarray
    n_acts: int = 0
    supervisors: list = field(default_factory=list)  # per behaviour: its AgxSupervisor entries, inner first
    backoff: list = field(default_factory=list)  # per behaviour: an AgxBackoff row per entry (min_backoff 0: a plain one) -> engine.set_backoff
    exception_classes: list = field(default_factory=list)  # the ExceptionTypes in use; the index is the class number
    spawn_sites: list = field(default_factory=list)  # (kind, word-0 base, word 1 or None: the parent's id) -> engine.set_children
    transparent_tags: tuple = ()  # the tags of the NotInfluenceReceiveTimeout message types -> engine.set_receive_timeout
    service_keys: list = field(default_factory=list)  # the ServiceKeys in use; the index is the key number -> engine.set_receptionist
    listing_types: dict = field(default_factory=dict)  # key number -> the MessageType of its Listing -> engine.set_listings
    hashed_keys: list = field(default_factory=list)  # the key numbers routed through by consistent hashing -> engine.set_router_logics
    virtual_nodes_factor: int = 0  # the hashed routers' virtualNodesFactor (0: none named one) -> engine.set_router_logics
    # (first_id, count, kind, word 0, word 1 or None: the entity's id, stop payload, idle delay, idle payload) -> engine.set_sharding
    entity_types: list = field(default_factory=list)

    @property
    def uses_supervision(self) -> bool:
        """A behaviour is supervised, throws or holds a PreRestart / PostStop case: the engine needs
        engine.set_supervision(tables.supervisors)."""
        return any(self.supervisors) or any(c.sig_code or isinstance(c.result, _Throw) for b in self.behaviors for c in b.cases)

    @property
    def uses_backoff(self) -> bool:
        """A supervisor restarts with backoff: the engine needs engine.set_backoff(tables.backoff) after
        engine.set_supervision(tables.supervisors)."""
        return any(r.min_backoff for row in self.backoff for r in row)

    @property
    def n_behaviors(self) -> int:
        return len(self.behaviors)

    @property
    def max_tells(self) -> int:
        """The most tells one message can emit (the largest tell count of any case): the engine's
        max_emit must be at least this (agx_set_behaviors rejects the tables otherwise)."""
        return max((sum(1 for i in range(c.act_first, c.act_first + c.act_count) if self.acts[i].op in (A_TELL, A_ROUTE, A_ASK_SEND))
                    for c in self.cases[:int(self.first[-1])]), default=0)

    @property
    def uses_forward(self) -> bool:
        """A tell or a route keeps the incoming message's sender (ref.forward, route(forward=True))."""
        return any(a.op in (A_TELL, A_ROUTE) and a.pad0 & ROUTE_KEEP_SENDER for a in self.acts[:self.n_acts])

    @property
    def uses_receptionist(self) -> bool:
        """The behaviours register, deregister, route, forward or read a listing: the engine needs
        engine.set_receptionist(len(tables.service_keys), capacity)."""
        return bool(self.service_keys) or self.uses_forward

    @property
    def uses_router_logics(self) -> bool:
        """A route is hashed or random: the engine needs engine.set_router_logics(tables.hashed_keys_mask,
        tables.virtual_nodes_factor, seed) after engine.set_receptionist."""
        return any(a.op == A_ROUTE and a.pad0 & (ROUTE_HASHED | ROUTE_RANDOM) for a in self.acts[:self.n_acts])

    @property
    def hashed_keys_mask(self) -> int:
        return sum(1 << k for k in self.hashed_keys)

    @property
    def uses_topics(self) -> bool:
        """The behaviours publish or name a Topic: the engine needs engine.set_topics(log_capacity) after
        engine.set_receptionist(len(tables.service_keys), capacity)."""
        return any(isinstance(k, Topic) for k in self.service_keys) or any(a.op == A_PUBLISH for a in self.acts[:self.n_acts])

    @property
    def uses_listings(self) -> bool:
        """The behaviours subscribe to or find a listing: the engine needs engine.set_listings(tables.listing_payloads)
        after engine.set_topics(log_capacity)."""
        return any(a.op in (A_SUBSCRIBE_LISTING, A_FIND) for a in self.acts[:self.n_acts])

    @property
    def listing_payloads(self) -> list:
        """Per service key the payload of its Listing envelope: the key's message type with the key number as the
        argument (0 for a key nobody subscribes to or finds)."""
        return [self.listing_types[k].payload(k) if k in self.listing_types else 0 for k in range(len(self.service_keys))]

    @property
    def stash_capacity(self) -> int:
        """The largest capacity of the stash buffers these behaviours use (0: none): the stash the
        actors' mailbox class needs (engine.set_stash)."""
        return max((c.result.buffer.capacity for b in self.behaviors for c in b.cases
                    if isinstance(c.result, (_StashEffect, _UnstashAll))), default=0)

    @property
    def timer_keys(self) -> int:
        """The timer slots per actor these behaviours need (0: no timers): engine.set_timers(tables.timer_keys)."""
        n = max((len(b.timers.keys) for b in self.behaviors if b.timers is not None), default=0)
        for a in self.acts[:self.n_acts]:
            if A_TIMER_SINGLE <= a.op <= A_TIMER_CANCEL_ALL:
                n = max(n, 1 if a.op == A_TIMER_CANCEL_ALL else a.word + 1)
            if a.op == A_ASK_ARM:
                n = max(n, a.word + 1)
        return n

    @property
    def uses_ask(self) -> bool:
        """The behaviours ask: the engine needs engine.set_ask() on top of engine.set_timers(tables.timer_keys)."""
        return any(a.op in (A_ASK_ARM, A_ASK_SEND) for a in self.acts[:self.n_acts])

    @property
    def uses_receive_timeout(self) -> bool:
        """The behaviours set or cancel a receive timeout: the engine needs engine.set_receive_timeout(
        tables.transparent_tags) on top of engine.set_timers(max(tables.timer_keys, 1))."""
        return any(a.op in (A_SET_RECEIVE_TIMEOUT, A_CANCEL_RECEIVE_TIMEOUT) for a in self.acts[:self.n_acts])

    @property
    def uses_sharding(self) -> bool:
        """The behaviours passivate or entity types are declared: the engine needs engine.set_sharding(
        tables.entity_types) on top of engine.set_receive_timeout."""
        return bool(self.entity_types) or any(a.op == A_PASSIVATE for a in self.acts[:self.n_acts])

    @property
    def uses_watch(self) -> bool:
        """The behaviours watch, unwatch or hold a signal case: the engine needs engine.set_death_watch(n)."""
        return any(c.signal and not c.sig_code for b in self.behaviors for c in b.cases) or \
            any(A_WATCH <= a.op <= A_UNWATCH for a in self.acts[:self.n_acts])

    @property
    def uses_children(self) -> bool:
        """The behaviours spawn, stop a child or read the spawn count: the engine needs engine.set_children(regions,
        tables.spawn_sites) on top of engine.set_death_watch(n)."""
        return any(a.op in (A_SPAWN, A_STOP_CHILD) or V_SPAWNED in (a.src, a.dsrc) or V_CHILD in (a.src, a.dsrc)
                   for a in self.acts[:self.n_acts]) or \
            any(s in (V_SPAWNED, V_CHILD) for c in self.cases[:int(self.first[-1])] for s in (c.src1, c.src2, c.src3, c.src4))

    @property
    def initial_timers(self) -> list:
        """with_timers' setup starts: (kind, key, periodic, delay, payload) -- actors registered with `kind`
        start timer `key` when they start (engine.start_timers on their range, before the first run)."""
        return [(KIND_COMPILED + i, *t) for i, b in enumerate(self.behaviors) for t in b.initial_timers]

    def kind_of(self, b: Behavior) -> int:
        """The actor kind that starts in behaviour `b`."""
        for i, x in enumerate(self.behaviors):
            if x is b:
                return KIND_COMPILED + i
        raise KeyError(b.name)


def _reachable(roots) -> list:
    seen, order = set(), []
    todo = list(roots)
    while todo:
        b = todo.pop(0)
        if id(b) in seen:
            continue
        seen.add(id(b))
        order.append(b)
        todo.extend(c.result for c in b.cases if isinstance(c.result, Behavior))
        todo.extend(c.result.target for c in b.cases
                    if isinstance(c.result, _UnstashAll) and isinstance(c.result.target, Behavior))
        todo.extend(e.site.behavior for c in b.cases for e in c.effects if isinstance(e, Action) and e.site is not None)
    return order


def compile_behaviors(roots, max_emit: int | None = None, transparent=(), entities=()) -> Tables:
    """Lower `roots` and every behaviour they become into the engine's tables.  With `max_emit`
    (the engine's agx_cfg.max_emit), a case that tells more often than that is a CompileError:
    the apply kernels reserve max_emit tell slots per message.  `transparent`: the MessageTypes that are
    NotInfluenceReceiveTimeout for behaviours with a receive timeout (Tables.transparent_tags).  `entities`: the
    Entity declarations of an engine with sharding (Tables.entity_types); their behaviours are lowered too."""
    entities = list(entities)
    for en in entities:
        if not isinstance(en, Entity):
            raise CompileError(f"entities= takes Entity declarations, not {en!r}")
        if en.stop_payload is None:
            raise CompileError(f"entity type {en.key.name!r} has no stop message (with_stop_message): context.passivate() "
                               "has nothing to send")
    if len(entities) > MAX_ENTITY_TYPES:
        raise CompileError(f"more than {MAX_ENTITY_TYPES} entity types")
    for i, en in enumerate(entities):
        for o in entities[:i]:
            if en.first_id < o.first_id + o.count and o.first_id < en.first_id + en.count:
                raise CompileError(f"the ranges of entity types {o.key.name!r} and {en.key.name!r} overlap")
    roots = list(roots) + [en.behavior for en in entities if not any(en.behavior is r for r in roots)]
    for mt in transparent:
        if not isinstance(mt, MessageType):
            raise CompileError(f"transparent= takes MessageTypes, not {mt!r}")
    behs = _reachable(roots)
    if len(behs) > MAX_BEHAVIORS:
        raise CompileError(f"more than {MAX_BEHAVIORS} behaviours")
    index = {id(b): i for i, b in enumerate(behs)}
    # the exception classes in use, numbered in order of appearance: thrown ones first, then the supervisors'
    excs = []
    for x in [c.result.exc for b in behs for c in b.cases if isinstance(c.result, _Throw)] + \
            [sv.exc for b in behs for sv in b.supervisors if sv.exc is not Throwable]:  # (the root: every bit)
        if not any(x is y for y in excs):
            excs.append(x)
    if len(excs) > MAX_EXCEPTION_CLASSES:
        raise CompileError(f"more than {MAX_EXCEPTION_CLASSES} exception classes")
    exc_id = {id(x): i for i, x in enumerate(excs)}
    cases, acts, first = [], [], [0]
    sites = []  # the spawn sites in use, in order of appearance: (behaviour index, base, word 1)
    skeys = []  # the service keys in use, in order of appearance
    ltypes = {}  # key number -> the MessageType of the key's Listing
    hkeys, vnfs = [], []  # the key numbers of the hashed routes; the virtualNodesFactors they name

    def key_no(key) -> int:
        if key not in skeys:
            if len(skeys) >= MAX_SERVICE_KEYS:
                raise CompileError(f"more than {MAX_SERVICE_KEYS} service keys")
            skeys.append(key)
        return skeys.index(key)

    def res_op(o: Operand) -> Operand:  # a listing operand's `word`: the key's number | the selector << 3
        return Operand(o.src, key_no(o.key) | (o.sel << 3), o.k) if isinstance(o, _KeyOperand) else o

    for b in behs:
        for c in b.cases:
            c_tests = [Test(x.cmp, res_op(x.lhs), res_op(x.rhs)) for x in c.tests]
            t = c_tests + [ALWAYS] * (2 - len(c_tests))
            res = c.result
            if isinstance(res, Behavior):
                code, nxt = RES_BECOME, index[id(res)]
            elif isinstance(res, _StashEffect):
                code, nxt = RES_STASH, 0
            elif isinstance(res, _UnstashAll):
                code, nxt = RES_UNSTASH_ALL, (index[id(res.target)] if isinstance(res.target, Behavior) else NEXT_SAME)
            elif isinstance(res, _Throw):
                code, nxt = RES_FAIL, exc_id[id(res.exc)]
            else:
                code, nxt = res.code, 0
            if c.signal:
                code |= CASE_SIGNAL
            n_acts_c = len(c.effects) + sum(1 for e in c.effects if e.ask is not None)  # (an ask lowers to ARM + SEND)
            if len(acts) + n_acts_c > 0xFFFF:
                raise CompileError("too many actions")
            cases.append(AgxCase(src1=t[0].lhs.src, word1=t[0].lhs.word, k1=t[0].lhs.k, cmp1=t[0].cmp,
                                 src2=t[0].rhs.src, word2=t[0].rhs.word, k2=t[0].rhs.k,
                                 src3=t[1].lhs.src, word3=t[1].lhs.word, k3=t[1].lhs.k, cmp2=t[1].cmp,
                                 src4=t[1].rhs.src, word4=t[1].rhs.word, k4=t[1].rhs.k,
                                 result=code, next=nxt, act_first=len(acts), act_count=n_acts_c))
            for e in c.effects:
                d = res_op(e.dst or Operand(V_CONST))
                if e.val is not res_op(e.val):
                    e = Action(e.op, e.word, res_op(e.val), e.dst, e.or_mask, e.site, e.into, e.key, e.flags, e.ask, e.listing, e.vnf)
                if e.op == A_SPAWN:  # dword: the site; pad0: the word `word` receives the child's id
                    key = (index[id(e.site.behavior)], e.site.base, e.site.word1)
                    if key not in sites:
                        if len(sites) >= MAX_SPAWN_SITES:
                            raise CompileError(f"more than {MAX_SPAWN_SITES} spawn sites")
                        sites.append(key)
                    acts.append(AgxAct(op=e.op, word=e.word, src=e.val.src, sword=e.val.word, k=e.val.k,
                                       dsrc=V_CONST, dword=sites.index(key), dk=0, pad0=1 if e.into else 0))
                    continue
                if e.op == A_ASK_ARM:  # ARM: the timeout message and the timeout; SEND: the request to the target
                    to, req, req_mask, adapt = e.ask
                    acts.append(AgxAct(op=A_ASK_ARM, word=e.word, src=e.val.src, sword=e.val.word, k=e.val.k,
                                       dsrc=d.src, dword=d.word, dk=d.k, or_mask=e.or_mask,
                                       pad0=0 if adapt is None else 1, pad1=0 if adapt is None else adapt))
                    acts.append(AgxAct(op=A_ASK_SEND, word=e.word, src=req.src, sword=req.word, k=req.k,
                                       dsrc=to.src, dword=to.word, dk=to.k, or_mask=req_mask))
                    continue
                if e.op in (A_SUBSCRIBE_LISTING, A_FIND):  # one Listing message type per key
                    kn = key_no(e.key)
                    if ltypes.setdefault(kn, e.listing) != e.listing:
                        raise CompileError(f"the Listing of {e.key!r} is {ltypes[kn]!r} and {e.listing!r}: one message type "
                                           "per key")
                if e.op == A_ROUTE and e.flags & ROUTE_HASHED:  # one virtualNodesFactor per engine
                    if key_no(e.key) not in hkeys:
                        hkeys.append(key_no(e.key))
                    if e.vnf and e.vnf not in vnfs:
                        vnfs.append(e.vnf)
                    if len(vnfs) > 1:
                        raise CompileError(f"two hashed routers with the virtualNodesFactors {vnfs[0]} and {vnfs[1]}: an "
                                           "engine has one")
                acts.append(AgxAct(op=e.op, word=e.word, src=e.val.src, sword=e.val.word, k=e.val.k,
                                   dsrc=d.src, dword=d.word, dk=d.k, or_mask=e.or_mask, pad0=e.flags,
                                   pad1=key_no(e.key) if e.key is not None else 0))
        first.append(len(cases))
    if len(cases) > MAX_CASES or len(acts) > MAX_ACTS:
        raise CompileError("tables too large")
    t = Tables(behs, (AgxCase * max(len(cases), 1))(*cases), (AgxAct * max(len(acts), 1))(*acts),
               np.asarray(first, dtype=np.uint32), len(acts))
    t.exception_classes = excs
    t.spawn_sites = [(KIND_COMPILED + bi, base, w1) for bi, base, w1 in sites]
    t.transparent_tags = tuple(sorted({mt.tag for mt in transparent}))
    t.service_keys = skeys
    t.listing_types = ltypes
    t.hashed_keys = sorted(hkeys)
    t.virtual_nodes_factor = vnfs[0] if vnfs else 0
    t.entity_types = [(en.first_id, en.count, KIND_COMPILED + index[id(en.behavior)], en.word0, en.word1, en.stop_payload,
                       en.idle[0], en.idle[1]) for en in entities]
    for b in behs:  # a supervisor of a class catches it and its descendants: the hierarchy as masks
        row = []
        for sv in b.supervisors:
            mask = 0xFFFFFFFF if sv.exc is Throwable else sum(1 << i for i, x in enumerate(excs) if x.is_a(sv.exc))
            e = AgxSupervisor(class_mask=mask, strategy=sv.strategy.kind, max_restarts=sv.strategy.max_restarts,
                              within=sv.strategy.within)
            if sv.strategy.kind == SUP_RESTART:
                for w, v in sv.reset.items():
                    e.reset_mask |= 1 << w
                    e.reset[w] = v
            row.append(e)
        t.supervisors.append(row)
        t.backoff.append([AgxBackoff(s.min_backoff, s.max_backoff, s.random_factor_q16, s.reset_after, s.stash_capacity)
                          if isinstance(s, _Backoff) else AgxBackoff() for s in (sv.strategy for sv in b.supervisors)])
    if t.uses_backoff and (t.uses_watch or t.timer_keys or t.stash_capacity):
        raise CompileError("restart_with_backoff lives on the supervision engine, which shares an engine with neither death "
                           "watch, timers nor a stash: the behaviours back off and use one of them")
    if t.uses_ask:  # on the timer engine: max_emit 1, the request is the case's one envelope
        if t.stash_capacity or t.uses_watch or t.uses_children or t.uses_supervision or t.uses_receptionist or \
                t.uses_receive_timeout or any(V_STASH in (a.src, a.dsrc) for a in acts) or \
                any(V_STASH in (c.src1, c.src2, c.src3, c.src4) for c in cases):
            raise CompileError("ask lives on the timer engine, which shares an engine with neither a stash, death watch, "
                               "children, supervision, the receptionist nor receive timeouts: the behaviours ask and use "
                               "one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"ask needs max_emit = 1, not {max_emit}")
        for c in cases:
            n = sum(1 for j in range(c.act_first, c.act_first + c.act_count) if acts[j].op in (A_TELL, A_ASK_SEND))
            if n > 1 and any(acts[j].op == A_ASK_SEND for j in range(c.act_first, c.act_first + c.act_count)):
                raise CompileError(f"a case holds {n} of tell and ask: an ask's request is the case's one envelope, and an "
                                   "engine with ask has max_emit 1")
    if t.uses_supervision:
        if t.uses_watch or t.timer_keys or t.stash_capacity or \
                any(V_STASH in (a.src, a.dsrc) for a in acts) or \
                any(V_STASH in (c.src1, c.src2, c.src3, c.src4) for c in cases):
            raise CompileError("supervision shares an engine with neither death watch, timers nor a stash: the behaviours "
                               "use supervision and one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"supervision needs max_emit = 1, not {max_emit}")
        for b in behs:
            if b.supervisors and any(c.result is b for x in behs if x is not b for c in x.cases):
                raise CompileError(f"behaviour {b.name!r} is supervised and reached by become: only an actor's initial "
                                   "behaviour can be supervised")
        for i, b in enumerate(behs):  # a failing or stopping case and a signal case share the message's tell slot
            tells = lambda c: sum(1 for j in range(c.act_first, c.act_first + c.act_count) if acts[j].op == A_TELL)
            fs = max((tells(cases[first[i] + j]) for j, c in enumerate(b.cases)
                      if not c.sig_code and (isinstance(c.result, _Throw) or c.result is Behaviors.stopped)), default=0)
            sg = max((tells(cases[first[i] + j]) for j, c in enumerate(b.cases) if c.sig_code), default=0)
            if fs + sg > 1:
                raise CompileError(f"behaviour {b.name!r}: a case that fails or stops and the largest PreRestart / PostStop "
                                   f"case tell {fs + sg} times together; an engine with supervision has max_emit 1")
    if t.uses_receive_timeout:  # on the timer engine: max_emit 1, tag 0xFB is the envelope's
        if t.stash_capacity or t.uses_watch or t.uses_children or t.uses_supervision or \
                any(V_STASH in (a.src, a.dsrc) for a in acts) or any(V_STASH in (c.src1, c.src2, c.src3, c.src4) for c in cases):
            raise CompileError("receive timeouts live on the timer engine, which shares an engine with neither a stash, death "
                               "watch, children nor supervision: the behaviours use a receive timeout and one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"receive timeouts need max_emit = 1, not {max_emit}")
        named = any(a.or_mask >> 24 == TAG_RECEIVE_TIMEOUT for a in acts) or TAG_RECEIVE_TIMEOUT in t.transparent_tags
        for c in cases:
            for s1, k1, cmp, s2, k2 in ((c.src1, c.k1, c.cmp1, c.src2, c.k2), (c.src3, c.k3, c.cmp2, c.src4, c.k4)):
                named |= cmp != CMP_ANY and ((s1 == V_TAG and k1 == 0 and s2 == V_CONST and k2 == TAG_RECEIVE_TIMEOUT) or
                                             (s2 == V_TAG and k2 == 0 and s1 == V_CONST and k1 == TAG_RECEIVE_TIMEOUT))
        if named:
            raise CompileError("message tag 0xFB is reserved for the receive-timeout envelope in behaviours that use a "
                               "receive timeout")
    if t.uses_sharding:  # on the receive-timeout engine: max_emit 1, a Passivate is the case's one envelope
        for c in cases:
            ops = [acts[j].op for j in range(c.act_first, c.act_first + c.act_count)]
            n = sum(1 for o in ops if o in (A_TELL, A_PASSIVATE, A_SPAWN, A_ASK_SEND))
            if A_PASSIVATE in ops and n > 1:
                raise CompileError(f"a case holds {n} of tell, spawn, ask and passivate: a Passivate sends the entity's stop "
                                   "message through the case's one envelope, and an engine with sharding has max_emit 1")
        if t.stash_capacity or t.uses_watch or t.uses_children or t.uses_supervision or t.uses_ask or t.uses_receptionist or \
                any(V_STASH in (a.src, a.dsrc) for a in acts) or any(V_STASH in (c.src1, c.src2, c.src3, c.src4) for c in cases):
            raise CompileError("sharding lives on the receive-timeout engine, which shares an engine with neither a stash, "
                               "death watch, children, supervision, ask nor the receptionist: the behaviours use sharding "
                               "and one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"sharding needs max_emit = 1, not {max_emit}")
        for en in entities:
            for pay, what in ((en.stop_payload, "stop"), (en.idle[1] if en.idle[0] else 0, "receive-timeout")):
                if pay >> 24 in (TAG_TIMER, TAG_RECEIVE_TIMEOUT):
                    raise CompileError(f"entity type {en.key.name!r}: its {what} message carries a reserved tag (0xFF, 0xFB)")
    if t.timer_keys or t.uses_receive_timeout:  # tag 0xFF is the TimerMsg's: no message type of these behaviours may carry it
        for a in acts:
            if a.or_mask >> 24 == TAG_TIMER:
                raise CompileError("message tag 0xFF is reserved for timer messages in behaviours that use timers")
        for c in cases:
            for s1, k1, cmp, s2, k2 in ((c.src1, c.k1, c.cmp1, c.src2, c.k2), (c.src3, c.k3, c.cmp2, c.src4, c.k4)):
                if cmp == CMP_EQ and ((s1 == V_TAG and k1 == 0 and s2 == V_CONST and k2 == TAG_TIMER) or
                                      (s2 == V_TAG and k2 == 0 and s1 == V_CONST and k1 == TAG_TIMER)):
                    raise CompileError("message tag 0xFF is reserved for timer messages in behaviours that use timers")
    if t.uses_watch:  # tag 0xFE is the Terminated envelope's: no message type of these behaviours may carry it
        if t.timer_keys:
            raise CompileError("death watch and timers do not share an engine: behaviours use one or the other")
        for a in acts:
            if a.or_mask >> 24 == TAG_WATCH:
                raise CompileError("message tag 0xFE is reserved for Terminated in behaviours that use death watch")
        for c in cases:
            for s1, k1, cmp, s2, k2 in ((c.src1, c.k1, c.cmp1, c.src2, c.k2), (c.src3, c.k3, c.cmp2, c.src4, c.k4)):
                if cmp == CMP_EQ and ((s1 == V_TAG and k1 == 0 and s2 == V_CONST and k2 == TAG_WATCH) or
                                      (s2 == V_TAG and k2 == 0 and s1 == V_CONST and k1 == TAG_WATCH)):
                    raise CompileError("message tag 0xFE is reserved for Terminated in behaviours that use death watch")
    if t.uses_children:  # on the death-watch engine: max_emit 1, tags 0xFD / 0xFC are the Create / Stop envelopes
        if t.timer_keys or t.stash_capacity or t.uses_supervision:
            raise CompileError("children live on the death-watch engine, which shares an engine with neither timers, a "
                               "stash nor supervision: the behaviours use children and one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"children need max_emit = 1, not {max_emit}")
        for c in cases:
            n = sum(1 for j in range(c.act_first, c.act_first + c.act_count) if acts[j].op in (A_TELL, A_SPAWN, A_STOP_CHILD))
            if n > 1:
                raise CompileError(f"a case holds {n} of tell, spawn and stop: each sends one envelope, and an engine "
                                   "with children has max_emit 1")
        for a in acts:
            if a.or_mask >> 24 in (TAG_CREATE, TAG_STOP):
                raise CompileError("message tags 0xFD and 0xFC are reserved for Create and Stop in behaviours that use children")
        for c in cases:
            for s1, k1, cmp, s2, k2 in ((c.src1, c.k1, c.cmp1, c.src2, c.k2), (c.src3, c.k3, c.cmp2, c.src4, c.k4)):
                if cmp != CMP_ANY and ((s1 == V_TAG and k1 == 0 and s2 == V_CONST and k2 in (TAG_CREATE, TAG_STOP)) or
                                       (s2 == V_TAG and k2 == 0 and s1 == V_CONST and k1 in (TAG_CREATE, TAG_STOP))):
                    raise CompileError("message tags 0xFD and 0xFC are reserved for Create and Stop in behaviours that use "
                                       "children")
    if t.uses_receptionist:  # an engine of its own: max_emit 1, a route goes through the case's tell slot
        if t.stash_capacity or t.timer_keys or t.uses_receive_timeout or t.uses_watch or t.uses_children or t.uses_supervision or \
                any(V_STASH in (a.src, a.dsrc) for a in acts) or any(V_STASH in (c.src1, c.src2, c.src3, c.src4) for c in cases):
            raise CompileError("the receptionist shares an engine with neither a stash, timers, death watch, children nor "
                               "supervision: the behaviours use the receptionist and one of them")
        if max_emit is not None and max_emit > 1:
            raise CompileError(f"the receptionist needs max_emit = 1, not {max_emit}")
        for c in cases:
            n = sum(1 for j in range(c.act_first, c.act_first + c.act_count) if acts[j].op in (A_TELL, A_ROUTE))
            if n > 1:
                raise CompileError(f"a case holds {n} of tell and route: each sends one envelope, and an engine with the "
                                   "receptionist has max_emit 1")
            p = sum(1 for j in range(c.act_first, c.act_first + c.act_count) if acts[j].op == A_PUBLISH)
            if p and n + p > 1:
                raise CompileError(f"a case holds {n + p} of tell, route and publish: a publication is the case's one "
                                   "envelope, and an engine with topics has max_emit 1")
    if t.uses_router_logics and (t.uses_topics or t.uses_listings):
        raise CompileError("hashed and random routes share an engine with neither topics nor listings: the behaviours use "
                           "router logics and one of them")
    if max_emit is not None and t.max_tells > max(1, max_emit):
        raise CompileError(f"a case tells {t.max_tells} times per message but max_emit is {max_emit}")
    return t


# ------------------------------------------------------------------ the built-in kinds, as typed behaviours
def library(ring_stride: int = 1) -> dict:
    """The engine's fixed behaviour kinds written in the DSL (used to cross-check the lowering
    against the hand-written kinds, include/akka_gpu.h agx_behavior_kind)."""
    st2 = State("count", "sum")
    counter = (ReceiveBuilder.create(st2)
               .on_any_message(lambda m, s: [s.count.inc(), s.sum.add(m.payload), Behaviors.same])
               .build("counter"))
    ring_state = State("count")
    ring = (ReceiveBuilder.create(ring_state)
            .on_any_message(lambda m, s: [s.count.inc(), self_ref(ring_stride).tell(m.payload - 1), Behaviors.same],
                            test=lambda m: m.payload > 0)
            .on_any_message(lambda m, s: [s.count.inc(), Behaviors.same])
            .build("ring"))
    sa = State("count", "limit")
    stop_after = (ReceiveBuilder.create(sa)
                  .on_any_message(lambda m, s: [s.count.inc(), Behaviors.stopped], when=lambda m, s: s.count + 1 >= s.limit)
                  .on_any_message(lambda m, s: [s.count.inc(), Behaviors.same])
                  .build("stop_after"))
    pp = State("left", "count")
    # BenchmarkActors.PingPong (akka-bench-jmh/src/main/scala/akka/actor/BenchmarkActors.scala:20-32)
    reply = lambda m, s: [s.count.inc(), m.sender.tell(m.payload), s.left.add(-1)]
    ping_pong = (ReceiveBuilder.create(pp)
                 .on_any_message(lambda m, s: reply(m, s) + [Behaviors.stopped], when=lambda m, s: s.left == 0)
                 .on_any_message(lambda m, s: reply(m, s) + [Behaviors.same])
                 .build("ping_pong"))
    return {"counter": counter, "ring": ring, "stop_after": stop_after, "ping_pong": ping_pong}


def echo(host_id: int) -> Behavior:
    """The observer of the reference's mailbox specs (`case x => testActor ! x`,
    akka-actor-tests/src/test/scala/akka/dispatch/ControlAwareDispatcherSpec.scala:50-52): every
    message is told on, payload unchanged, to the host-side actor `host_id` (agx_set_outbound), so
    the outbox shows the order in which the mailbox handed the messages out."""
    st = State("count", "last")
    return (ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [s.count.inc(), s.last.set(m.payload), actor_ref(host_id).tell(m.payload),
                                          Behaviors.same])
            .build("echo"))


def forwarder(n_actors: int, hop: int, stop_tag: int) -> Behavior:
    """A tagged-message relay: a message with tag `stop_tag` stops the actor; a message from a
    host-side sender (id >= n_actors) is echoed to it; any other message with a hop count (its
    24-bit argument) above 0 goes on to the actor `hop` ids further with one hop less, tag kept.
    State: messages handled, the last payload handled (order-sensitive)."""
    st = State("count", "last")
    seen = lambda m, s: [s.count.inc(), s.last.set(m.payload)]
    return (ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [s.count.inc(), Behaviors.stopped], test=lambda m: m.tag == stop_tag)
            .on_any_message(lambda m, s: seen(m, s) + [m.sender.tell(m.payload), Behaviors.same],
                            test=lambda m: m.sender.dst >= n_actors)
            .on_any_message(lambda m, s: seen(m, s) + [self_ref(hop).tell(m.payload - 1), Behaviors.same],
                            test=lambda m: m.arg > 0)
            .on_any_message(lambda m, s: seen(m, s) + [Behaviors.same])
            .build(f"forwarder{hop}"))


SWITCH_ON, SWITCH_OFF, PING = MessageType("SwitchOn", 1), MessageType("SwitchOff", 2), MessageType("Ping", 3)


def switch() -> Behavior:
    """Two behaviours that become each other (TY/Behavior.scala:150): `off` counts a SwitchOn and
    becomes `on`, leaves Ping unhandled; `on` sums Ping arguments, answers Ping(n) with Ping(n - 1)
    while n > 0, and becomes `off` on SwitchOff."""
    st = State("flips", "sum")
    on, off = Behavior("on", st), Behavior("off", st)
    (ReceiveBuilder.create(st)
     .on_message(SWITCH_ON, lambda m, s: [s.flips.inc(), on])
     .on_message(SWITCH_OFF, lambda m, s: [Behaviors.same])
     .build(into=off))
    (ReceiveBuilder.create(st)
     .on_message(SWITCH_OFF, lambda m, s: [s.flips.inc(), off])
     .on_message(PING, lambda m, s: [s.sum.add(m.arg), m.sender.tell(PING(m.arg - 1)), Behaviors.same],
                 test=lambda m: m.arg > 0)
     .on_message(PING, lambda m, s: [Behaviors.same])
     .build(into=on))
    return off
