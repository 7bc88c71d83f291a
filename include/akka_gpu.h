/*
 * akka_gpu.h — C ABI of the MI355X batched actor-dispatch engine.
 *
 * This is the drop-in boundary for Akka's Dispatcher/Mailbox hot loop
 * (SURVEY.md §8(b)).  A JVM host (JNI or Panama) or the
 * Python host in akka_amd/ binds exactly these symbols.  Plain C types only:
 * no torch, no HIP types, no exceptions cross this boundary; every function
 * returns an agx_status (0 = OK).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to /root/reference, aliases as in SURVEY.md):
 *
 *   agx_create          <- MessageDispatcherConfigurator.dispatcher() +
 *                          Dispatchers.configuratorFrom
 *                          (akka-actor/src/main/scala/akka/dispatch/AbstractDispatcher.scala:338-347,
 *                           akka-actor/src/main/scala/akka/dispatch/Dispatchers.scala:235-262)
 *                          with MailboxType.create for the bounded/unbounded queue
 *                          (akka-actor/src/main/scala/akka/dispatch/Mailbox.scala:638-640,
 *                           akka-actor/src/main/scala/akka/dispatch/Mailboxes.scala:204-260)
 *   agx_register_range  <- MessageDispatcher.attach / ActorCell.init (Create) for a
 *                          contiguous range of fixed-layout actors
 *                          (AbstractDispatcher.scala:145-148, akka-actor/.../actor/dungeon/Dispatch.scala:63-100)
 *   agx_stage_tells     <- LocalActorRef.! -> ActorCell.sendMessage -> Dispatcher.dispatch
 *                          (akka-actor/.../actor/ActorRef.scala:412-413, ActorCell.scala:325-326,
 *                           akka-actor/.../dispatch/Dispatcher.scala:61-65)
 *   agx_run             <- registerForExecution + Mailbox.run/processMailbox on the
 *                          ForkJoinPool, as BSP supersteps
 *                          (Dispatcher.scala:120-143, Mailbox.scala:227-277)
 *   agx_read_state      <- (no reference counterpart: actor state is private to the
 *                          JVM object; the GPU engine exposes it for the host/oracle)
 *   agx_set_mailbox_class / agx_set_mailbox
 *                       <- Mailboxes.lookupConfigurator / getMailboxType per actor
 *                          (akka-actor/.../dispatch/Mailboxes.scala:140-191,204-260)
 *   agx_set_mailbox_priority
 *                       <- UnboundedPriorityMailbox / UnboundedStablePriorityMailbox and their bounded
 *                          forms, UnboundedControlAwareMailbox / BoundedControlAwareMailbox
 *                          (akka-actor/.../dispatch/Mailbox.scala:726-816, 867-1025)
 *   agx_set_outbound / agx_take_outbound
 *                       <- sender() ! reply to a JVM actor (akka-actor/.../actor/ActorCell.scala:583-587):
 *                          GPU tells to host-side actors leave the engine through an outbox
 *   agx_destroy         <- MessageDispatcher.shutdown (AbstractDispatcher.scala:325)
 *
 * Threading: an engine handle is driven by one host thread at a time (the
 * single-writer-per-actor rule at engine granularity, Mailbox.scala:185-203) -- except agx_tell,
 * which any thread may call at any time (the lock-free tell path, below).
 */
#ifndef AKKA_GPU_H
#define AKKA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_ABI_VERSION 1u

typedef int32_t agx_status;
#define AGX_OK 0
#define AGX_EINVAL 1    /* bad argument / configuration                     */
#define AGX_ENOMEM 2    /* device or host allocation failed                 */
#define AGX_EDEVICE 3   /* HIP runtime error (message via agx_last_error)   */
#define AGX_ECOMM 4     /* RCCL error                                       */
#define AGX_ECAPACITY 5 /* in-flight messages exceed the engine's capacity  */
#define AGX_ESTATE 6    /* call not valid in the engine's current state     */
#define AGX_ERANGE 7    /* a GCounter / PNCounter slot passed 2^64 - 1: the reference's BigInt
                           (DD/GCounter.scala:53) has no bound, the u64 slot wrapped; or an ORSet
                           replica's own version passed 2^32 - 1: the reference's Long version
                           (DD/VersionVector.scala:76-80) does not wrap, the u32 entry did */

/* "no sender" (Actor.noSender / deadLetters as sender, AbstractDispatcher.scala:29-37) */
#define AGX_NO_SENDER 0xFFFFFFFFu

/* Behaviour kinds: the fixed-layout subset of typed Behaviors.receive
 * (akka-actor-typed/.../scaladsl/Behaviors.scala:101-121).  Each returns
 * same / stopped / unhandled (TY/Behavior.scala:229-278,
 * TY/internal/adapter/ActorAdapter.scala:152-168).  State words are u64.   */
enum agx_behavior_kind {
  AGX_KIND_NONE = 0,       /* unregistered: every message is a dead letter            */
  AGX_KIND_COUNTER = 1,    /* w0 += 1; w1 += payload                                  */
  AGX_KIND_RING = 2,       /* w0 += 1; payload>0 -> tell((self+stride)%N, payload-1)  */
  AGX_KIND_FANOUT = 3,     /* w0 += 1; w1 += payload; ttl=pay>>24 >0 -> k Zipf tells  */
  AGX_KIND_FORWARD_RR = 4, /* w0 += 1; payload>0 -> tell(next out-edge RR, payload-1) */
  AGX_KIND_STOP_AFTER = 5, /* w0 += 1; w0 >= w1 -> Behaviors.stopped                  */
  AGX_KIND_PINGPONG = 6,   /* BenchmarkActors.PingPong: reply to sender, stop at 0    */
  AGX_KIND_EVEN = 7,       /* odd payload -> Behaviors.unhandled; else w0 += 1         */
  /* Replicator-style CRDT replicas (akka-distributed-data), see "CRDT behaviours" below */
  AGX_KIND_GCOUNTER = 8,   /* w[0..7]  = GCounter slots                                 */
  AGX_KIND_PNCOUNTER = 9,  /* w[0..7]  = increments, w[8..15] = decrements              */
  AGX_KIND_ORSET = 10,     /* w[0..259] = 64 x 8 u32 dots + 8 u32 version vector        */
  AGX_KIND_MAX = 11
};

/* Behaviour results (ActorAdapter.next, TY/internal/adapter/ActorAdapter.scala:152-168) */
#define AGX_RES_SAME 0u
#define AGX_RES_STOPPED 1u
#define AGX_RES_UNHANDLED 2u
#define AGX_RES_BECOME 3u /* compiled behaviours: the next behaviour is agx_case.next */
/* compiled behaviours of a deque-based mailbox class (agx_set_stash; StashBuffer, TY/internal/
 * StashBufferImpl.scala:61-79,131-218):
 *   AGX_RES_STASH        the case's actions run, then the message is appended to the actor's stash
 *                        buffer (buffer.stash(msg); a full buffer is StashOverflowException: the actor stops);
 *   AGX_RES_UNSTASH_ALL  buffer.unstashAll(next): the behaviour becomes agx_case.next
 *                        (AGX_NEXT_SAME: it stays) and the buffered messages are released.            */
#define AGX_RES_STASH 4u
#define AGX_RES_UNSTASH_ALL 5u
#define AGX_NEXT_SAME 0xFFu /* agx_case.next of AGX_RES_UNSTASH_ALL: Behaviors.same */
/* compiled behaviours of an engine with supervision (agx_set_supervision): the handler throws.  The case's
 * actions run first (the effects before the throw), the message counts as delivered, and agx_case.next is the
 * exception class, 0..AGX_MAX_EXCEPTION_CLASSES - 1. */
#define AGX_RES_FAIL 6u
#define AGX_MAX_EXCEPTION_CLASSES 32u

/* --- compiled behaviours ------------------------------------------------------
 * A typed Behaviors.receiveMessage / javadsl ReceiveBuilder subset lowered to tables
 * (akka_amd/typed.py is the lowering; TY/scaladsl/Behaviors.scala:101-121,
 * TY/javadsl/ReceiveBuilder.scala:48-98,209-218).  An actor of kind AGX_KIND_COMPILED + b
 * runs behaviour b: cases [first[b], first[b+1]) are tried in order and the first whose
 * message tests and state guard hold runs its actions, then returns its result --
 * Behaviors.same, stopped, unhandled, or a become to behaviour `next` (stored in the
 * actor's kind byte).  No matching case = Behaviors.unhandled (ReceiveBuilder.receive).
 * Compiled behaviours keep their state in words 0 and 1 (two u64 fields).
 * Operands: value = base(src, word) + k, base = 0 (AGX_V_CONST), the payload, its tag
 * (payload >> 24), its argument (payload & 0xFFFFFF), state word `word`, the sender id or
 * the actor's own id.  Comparisons are unsigned 64-bit.                              */
#define AGX_KIND_COMPILED 16u
/* an LWWMap replica (see "LWWMap replicas" below).  Not in enum agx_behavior_kind and above
 * AGX_KIND_MAX: agx_register_range accepts it explicitly, and code that only knows the enum keeps
 * refusing it. */
#define AGX_KIND_LWWMAP 11u
/* a PNCounterMap replica (see "PNCounterMap replicas" below); outside the enum for the same reason */
#define AGX_KIND_PNCOUNTERMAP 12u
/* an ORMultiMap replica (see "ORMultiMap replicas" below); outside the enum for the same reason */
#define AGX_KIND_ORMULTIMAP 13u
#define AGX_MAX_BEHAVIORS 64u
#define AGX_MAX_CASES 1024u
#define AGX_MAX_ACTS 4096u
enum agx_operand { AGX_V_CONST = 0, AGX_V_PAYLOAD = 1, AGX_V_TAG = 2, AGX_V_ARG = 3, AGX_V_WORD = 4,
                   AGX_V_SENDER = 5, AGX_V_SELF = 6,
                   AGX_V_STASH = 7 /* the size of the actor's stash buffer (StashBuffer.size); 0 on an
                                      engine without a deque-based mailbox class (agx_set_stash) */,
                   AGX_V_TIMER = 8 /* 1 if the actor's timer slot `word` (the key) is active, else 0
                                      (TimerScheduler.isTimerActive); engines with timers (agx_set_timers) */,
                   /* engines with children (agx_set_children): */
                   AGX_V_SPAWNED = 9 /* the actor's spawn count */,
                   AGX_V_CHILD = 10 /* the id of child number (value + k) mod spawn count of the actor; value =
                                       state word `word` (0, 1) or 0 (word = AGX_CHILD_NO_WORD); 0xFFFFFFFF with no
                                       children */,
                   /* engines with the receptionist (agx_set_receptionist); `word` = key | selector << 3: */
                   AGX_V_LISTING_SIZE = 11 /* the size of the listing of key `word & 7` in force this tick */,
                   AGX_V_SERVICE_AT = 12 /* listing[x mod size] of key `word & 7`, x = the value the selector names
                                            (AGX_SVC_WORD0 / WORD1: that state word, AGX_SVC_ARG: the message's
                                            argument, AGX_SVC_CONST: 0) + k; 0xFFFFFFFF when the listing is empty */ };
#define AGX_CHILD_NO_WORD 2u
#define AGX_SVC_WORD0 0u
#define AGX_SVC_WORD1 1u
#define AGX_SVC_ARG 2u
#define AGX_SVC_CONST 3u
#define AGX_SVC_WORD(key, sel) ((uint8_t)((key) | ((sel) << 3)))
enum agx_cmp { AGX_CMP_ANY = 0, AGX_CMP_EQ = 1, AGX_CMP_NE = 2, AGX_CMP_LT = 3, AGX_CMP_LE = 4, AGX_CMP_GT = 5,
               AGX_CMP_GE = 6 };
enum agx_action_op {
  AGX_A_SET = 1,  /* word[w] = operand                                          */
  AGX_A_ADD = 2,  /* word[w] += operand (wrapping)                              */
  AGX_A_MAX = 3,  /* word[w] = max(word[w], operand)                            */
  AGX_A_MIN = 4,
  AGX_A_TELL = 5, /* tell(dst operand, payload): payload = (u32)operand, or with a message tag
                     (or_mask != 0) (operand & 0xFFFFFF) | or_mask; a dst operand based on the
                     actor's own id is taken mod n_actors (ring neighbours); an unknown id is a
                     dead letter */
  /* Timer actions (engines with timers, agx_set_timers; TimerScheduler, TY/internal/TimerSchedulerImpl.scala:
   * 61-172).  `word` is the key (the slot index); the timer's message payload is the operand as a TELL's
   * payload ((u32)operand, or (operand & 0xFFFFFF) | or_mask); the delay in ticks is the d-operand (dsrc,
   * dword, dk), where a TELL has its destination: below 1 it counts as 1, above 2^31 - 1 it is clamped. */
  AGX_A_TIMER_SINGLE = 6,     /* startSingleTimer(key, msg, delay)                                       */
  AGX_A_TIMER_PERIODIC = 7,   /* startTimerWithFixedDelay / startTimerAtFixedRate (they coincide: 2.3) */
  AGX_A_TIMER_CANCEL = 8,     /* cancel(key)                                                             */
  AGX_A_TIMER_CANCEL_ALL = 9, /* cancelAll()                                                             */
  /* Death watch actions (engines with death watch, agx_set_death_watch; AA/dungeon/DeathWatch.scala:19-113).
   * The ref is the d-operand (dsrc, dword, dk), where a TELL has its destination: a ref based on the actor's
   * own id wraps mod n_actors, as a TELL's does.  WATCH_WITH's custom message is the operand as a TELL's
   * payload ((u32)operand, or (operand & 0xFFFFFF) | or_mask). */
  AGX_A_WATCH = 10,      /* context.watch(ref)          (DeathWatch.scala:23-34)  */
  AGX_A_WATCH_WITH = 11, /* context.watchWith(ref, msg) (DeathWatch.scala:36-47)  */
  AGX_A_UNWATCH = 12,    /* context.unwatch(ref)        (DeathWatch.scala:49-60)  */
  /* Children (engines with children, agx_set_children).  SPAWN: `dword` is the spawn site, the operand (src, sword,
   * k) is the argument, whose low AGX_SPAWN_ARG_BITS bits are added to the site's word-0 base; with pad0 & 1 the
   * state word `word` receives the child's id, 0xFFFFFFFF when the spawn is refused.  STOP_CHILD: the ref is the
   * d-operand, as a WATCH's.  Each sends one envelope through the case's tell slot: with max_emit = 1 a case
   * holds at most one of TELL, SPAWN and STOP_CHILD. */
  AGX_A_SPAWN = 13,      /* context.spawn(site behaviour) (TY/scaladsl/ActorContext.scala spawnAnonymous) */
  AGX_A_STOP_CHILD = 14, /* context.stop(ref)           (ActorContextAdapter.scala:79-106) */
  /* Receive timeouts (engines with receive timeouts, agx_set_receive_timeout; AA/dungeon/ReceiveTimeout.scala:
   * 18-74).  SET: the message payload is the operand as a TELL's payload, the delay in ticks is the d-operand,
   * as a timer's (below 1 it counts as 1, above 2^31 - 1 it is clamped; a constant below 1 is refused). */
  AGX_A_SET_RECEIVE_TIMEOUT = 15,   /* context.setReceiveTimeout(delay, msg) (ActorContextAdapter.scala:120-126) */
  AGX_A_CANCEL_RECEIVE_TIMEOUT = 16, /* context.cancelReceiveTimeout()        (ActorContextAdapter.scala:128-131) */
  /* The receptionist (engines with the receptionist, agx_set_receptionist).  The service key is
   * pad1.  REGISTER / DEREGISTER set / clear the actor's own bit of the key.  ROUTE is selectRoutee(msg) ! msg: the
   * payload is the operand as a TELL's; pad0 & AGX_ROUTE_KEEP_SENDER keeps the incoming message's sender on the
   * envelope (a forward), else the sender is the router; pad0 & AGX_ROUTE_BY_INDEX takes listing[x mod size] with
   * x the d-operand (dsrc, dword, dk), else round robin with the cursor in state word `word`.  A ROUTE sends
   * through the case's tell slot: a case holds at most one of TELL and ROUTE.  AGX_ROUTE_KEEP_SENDER on a plain
   * AGX_A_TELL (ref.forward(msg)) is accepted on an engine with the receptionist only.  On an engine with router
   * logics (agx_set_router_logics) pad0 & AGX_ROUTE_HASHED takes nodeFor(stringHash(str(x))) of the
   * key's hash ring, x the low 32 bits of the d-operand; pad0 & AGX_ROUTE_RANDOM takes listing[r mod size] with r
   * drawn from the counter in state word `word`, which then grows by one.  BY_INDEX, HASHED and RANDOM exclude one
   * another (agx_run refuses tables that set two of them on one action). */
  AGX_A_REGISTER = 17,   /* receptionist ! Register(key, self)   (LocalReceptionist.scala:147-175) */
  AGX_A_DEREGISTER = 18, /* receptionist ! Deregister(key, self) (LocalReceptionist.scala:177-199) */
  AGX_A_ROUTE = 19,      /* group router: selectRoutee(msg) ! msg (GroupRouterImpl.scala:114-146) */
  /* The ask pattern (engines with ask, agx_set_ask).  context.ask lowers to ARM directly followed by
   * the SEND of the same key.  ARM: `word` is the key; the operand and or_mask hold the timeout message as a
   * TIMER_SINGLE's, the d-operand is the timeout in ticks as a timer's delay; pad0 & 1: the reply's tag is replaced
   * by pad1 (the adapt tag).  SEND: a TELL's layout with `word` = the key; its envelope carries the ask ref as the
   * sender.  It is the case's one envelope: a case holds at most one of TELL and ASK_SEND. */
  AGX_A_ASK_ARM = 20,    /* context.ask: the promise ref and its timeout task (AskPattern.scala:109-162) */
  AGX_A_ASK_SEND = 21,   /* context.ask: target ! createRequest(ref) (ActorContextImpl.scala:203-218) */
  /* Pub-sub topics (engines with topics, agx_set_topics).  PUBLISH is topic ! Publish(msg): pad1 is
   * the key (the topic), pad0 must be 0, the payload is the operand as a TELL's, there is no destination.  The
   * envelope every subscriber receives in the next tick carries the publisher as its sender.  A case holds at most
   * one of TELL, ROUTE and PUBLISH. */
  AGX_A_PUBLISH = 22,    /* topic ! Topic.Publish(msg) (TopicImpl.scala:60-143) */
  /* Subscribe / Find and the Listing message (engines with listings, agx_set_listings).  pad1 is the
   * key, pad0 must be 0; an actor subscribes or asks for itself only.  Neither is an envelope of the case: a case may
   * hold them beside its one TELL, ROUTE or PUBLISH. */
  AGX_A_SUBSCRIBE_LISTING = 23, /* receptionist ! Subscribe(key, self) (LocalReceptionist.scala:213-220) */
  AGX_A_FIND = 24,              /* receptionist ! Find(key, self)      (LocalReceptionist.scala:209-211) */
  /* Sharded entities (engines with sharding, agx_set_sharding).  PASSIVATE is shard !
   * Passivate(context.self): the entity is marked passivating and its type's stop message goes to the entity itself
   * through the case's tell slot (sender = the entity); no operand is read.  A case holds at most one of TELL and
   * PASSIVATE. */
  AGX_A_PASSIVATE = 25          /* context.passivate(): shard ! Passivate(self) (Shard.scala:405-417) */
};
/* The ask ref: AGX_ASK_REF_BIT | key << 29 | (generation mod 2^7) << 22 | the asker's id. */
#define AGX_ASK_REF_BIT 0x80000000u
#define AGX_ASK_REF_KEY_SHIFT 29u
#define AGX_ASK_REF_GEN_SHIFT 22u
#define AGX_ASK_REF_GEN_MASK 0x7Fu
#define AGX_ASK_REF_ID_MASK 0x3FFFFFu
#define AGX_ASK_MAX_ACTORS 0x3FFFFFu /* an engine with ask has at most 2^22 - 1 actors: the ref carries the id */
#define AGX_ROUTE_KEEP_SENDER 1u
#define AGX_ROUTE_BY_INDEX 2u
#define AGX_ROUTE_HASHED 4u
#define AGX_ROUTE_RANDOM 8u
#define AGX_MAX_VIRTUAL_NODES 64u
#define AGX_MAX_RING_POINTS (1u << 24)
#define AGX_MAX_SERVICE_KEYS 8u
#define AGX_TAG_RECEIVE_TIMEOUT 0xFBu /* the message tag of a receive-timeout envelope: reserved on an engine with
                                         receive timeouts */
#define AGX_TAG_CREATE 0xFDu    /* the message tag of a Create envelope: reserved on an engine with children */
#define AGX_TAG_STOP 0xFCu      /* the message tag of a Stop envelope: reserved on an engine with children */
#define AGX_MAX_CHILD_REGIONS 8u
#define AGX_MAX_ENTITY_TYPES 8u
#define AGX_ENTITY_WORD1_ID 1u  /* agx_entity_type.flags: state word 1 starts as the entity's id, not as `word1` */
#define AGX_MAX_SPAWN_SITES 64u
#define AGX_SPAWN_ARG_BITS 18u  /* a Create's payload: AGX_TAG_CREATE << 24 | site << 18 | argument */
#define AGX_SPAWN_ARG_MASK 0x3FFFFu
#define AGX_TAG_TIMER 0xFFu     /* the message tag (payload >> 24) of a TimerMsg: reserved on an engine with timers */
#define AGX_MAX_TIMER_KEYS 4u
#define AGX_TAG_WATCH 0xFEu     /* the message tag of a Terminated envelope: reserved on an engine with death watch */
#define AGX_MAX_WATCH_SLOTS 4u
/* agx_case.result flag: the case is a signal case (typed receiveSignal).  Ordinary messages skip signal cases,
 * signals try only them.  Inside a signal case the payload reads as AGX_SIGNAL_TERMINATED and AGX_V_SENDER is
 * the terminated ref (TY/internal/adapter/ActorAdapter.scala:84-91,134-138). */
#define AGX_CASE_SIGNAL 0x80u
#define AGX_SIGNAL_TERMINATED 0xFE000001u
/* The signals of an engine with supervision (agx_set_supervision).  A signal case of these tests the payload:
 * its first test is AGX_V_PAYLOAD (k 0) AGX_CMP_EQ AGX_V_CONST (k = the signal).  Such a case is a supervision
 * signal case; every other signal case belongs to death watch.  AGX_V_SENDER is the actor itself. */
#define AGX_SIGNAL_PRERESTART 0xFE000002u
#define AGX_SIGNAL_POSTSTOP 0xFE000003u
typedef struct agx_case {
  uint8_t src1, word1, cmp1, src2; /* test 1: operand(src1, word1, k1) cmp1 operand(src2, word2, k2) */
  uint8_t word2, src3, word3, cmp2; /* test 2: operand(src3, word3, k3) cmp2 operand(src4, word4, k4) */
  uint8_t src4, word4, result, next;
  uint16_t act_first, act_count;    /* actions [act_first, act_first + act_count) */
  int64_t k1, k2, k3, k4;
} agx_case; /* 48 B */
typedef struct agx_act {
  uint8_t op, word, src, sword;     /* action; target word; operand (src, sword, k)  */
  uint8_t dsrc, dword, pad0, pad1;  /* AGX_A_TELL destination operand (dsrc, dword, dk) */
  uint32_t or_mask;                 /* AGX_A_TELL: payload |= or_mask (a message tag)  */
  int64_t k, dk;
} agx_act; /* 32 B */

#define AGX_MAX_WORDS 2576u /* = AGX_ORMM_WORDS (the widest layout: an engine of ORMultiMap replicas, exactly this) */
#define AGX_MAX_GENERAL_WORDS 1296u /* = AGX_PNCMAP_WORDS: n_words of every other engine is 1..this; the widths
                                     * between the two fit no layout and are refused                            */
#define AGX_MAX_RANKS 16u

/* --- CRDT behaviours ---------------------------------------------------------
 * Each actor of a CRDT kind is one replica holding one data value; its node
 * index (the UniqueAddress slot, akka-cluster/.../Member.scala:307-311) is
 * id % AGX_CRDT_NODES.  Two message shapes:
 *  - control tells: payload = (op << 24) | arg, from the host or from itself
 *      AGX_OP_INCREMENT  arg = n    GCounter.increment / PNCounter.increment
 *                                   (DD/GCounter.scala:97-111, DD/PNCounter.scala:161-176)
 *      AGX_OP_DECREMENT  arg = n    PNCounter.decrement (:167-176)
 *      AGX_OP_ADD        arg = e    ORSet.add (DD/ORSet.scala:339-351), e < 64
 *      AGX_OP_REMOVE     arg = e    ORSet.remove (:380-387)
 *      AGX_OP_CLEAR                 ORSet.clear (:404-412)
 *      AGX_OP_GOSSIP     arg = k    Replicator GossipTick (DD/Replicator.scala:1316,2029-2061):
 *                                   send the full state to `fanout` random peers
 *                                   and, if k > 0, GOSSIP(k-1) to itself
 *  - state gossip: a full-state snapshot; the receiver merges it
 *    (GCounter.merge :113-125, PNCounter.merge :178, ORSet.merge :427-452).
 *    On the wire the sender field carries AGX_WIDE_BIT and the payload is
 *    (data type << 30) | an engine-internal handle to the snapshot (type =
 *    kind - AGX_KIND_GCOUNTER).  A gossip of another data type, and any state
 *    gossip reaching a non-CRDT behaviour, is Behaviors.unhandled.  Host
 *    tells are always control tells.
 * Unknown ops are Behaviors.unhandled.                                       */
#define AGX_CRDT_NODES 8u
#define AGX_ORSET_ELEMS 64u
#define AGX_GCOUNTER_WORDS 8u
#define AGX_PNCOUNTER_WORDS 16u
#define AGX_ORSET_WORDS 260u /* (64 * 8 + 8) u32 */
#define AGX_WIDE_BIT 0x80000000u
#define AGX_OP_INCREMENT 1u
#define AGX_OP_DECREMENT 2u
#define AGX_OP_ADD 3u
#define AGX_OP_REMOVE 4u
#define AGX_OP_CLEAR 5u
#define AGX_OP_GOSSIP 6u
#define AGX_OP_DELTA_TICK 7u
#define AGX_OP(op, arg) (((uint32_t)(op) << 24) | ((uint32_t)(arg) & 0xFFFFFFu))

/* --- delta-CRDT replication (agx_set_delta_crdt; Replicator delta-crdt.enabled) --------
 * Replicas form keys of AGX_CRDT_NODES consecutive ids (key = id / 8, node = id % 8): the
 * 8 replicas of a key are the key's DataEnvelopes on 8 Replicator nodes, and gossip (full
 * state and deltas) only flows between them.  Each replica's state words are the data
 * words followed by the envelope/selector area and a delta log (u32 view, D = data words):
 *   u32[2D + 0..7]    DataEnvelope.deltaVersions (seqNr last applied per node; DD/Replicator.scala:910-917)
 *   u32[2D + 8]       DeltaPropagationSelector.deltaCounter  (DD/DeltaPropagationSelector.scala:44-57)
 *   u32[2D + 9]       deltaNodeRoundRobinCounter
 *   u32[2D + 10..17]  deltaSentToNode per node (0 = nothing sent)
 *   deltaEntries --
 *     counters, u32[2D + 24 ..+ AGX_COUNTER_DELTA_U32]: {seqNr, value lo, hi} of the last increments
 *       delta, the same of the last decrements delta, the last NoDeltaPlaceholder's seqNr, 0.  A
 *       counter delta is the updated slot's new value and the own slots never decrease, so the
 *       slot-max merge of the deltas after any seqNr j is these last deltas (or a placeholder if
 *       one lies after j): unbounded, as the reference's map (DD/DeltaPropagationSelector.scala:149-155).
 *     ORSet, u32[2D + 24 + AGX_DELTA_LOG_U32(1) * (seq % AGX_DELTA_LOG) ...], a ring:
 *       {seq, type (1 AddDeltaOp, 2 RemoveDeltaOp, 3 FullStateDeltaOp) | elem << 8, version, 0, vvector[8]};
 *       an ORSet replica that would overwrite a seqNr some node has not been sent reports
 *       AGX_ECAPACITY (the one bounded difference from the reference).
 * Ops on a delta replica:
 *   AGX_OP_DELTA_TICK  arg = k | AGX_DELTA_WRITE?   DeltaPropagationTick (DD/Replicator.scala:1953-1963):
 *       (AGX_DELTA_WRITE: first tell itself one seeded local update -- a writer client), then for
 *       each node of this tick's round-robin slice with deltas after deltaSentToNode, merge them
 *       into one delta group (DeltaOp.merge, max-delta-size) and tell that replica a
 *       DeltaPropagation(fromSeqNr, toSeqNr); if k > 0, DELTA_TICK(k-1) to itself.
 *   a DeltaPropagation is applied with causal delivery for ORSet (skip if already handled or a
 *   seqNr is missing, DD/Replicator.scala:1965-2027) and ORSet.mergeDelta (DD/ORSet.scala:455-501);
 *   counters merge it (no causal delivery needed).  A group that is a NoDeltaPlaceholder
 *   (too large, or a no-op update in range) is not told (createDeltaPropagation leaves it out,
 *   DD/Replicator.scala:1364,1957); deltaSentToNode still advances.                           */
#define AGX_DELTA_WRITE 0x800000u
#define AGX_DELTA_LOG 64u            /* ORSet ring entries per replica (seqNrs not yet sent to every node) */
#define AGX_COUNTER_DELTA_U32 8u     /* counters: the last delta per slot + the last placeholder      */
#define AGX_DELTA_ENV_WORDS 12u      /* u64 words of the envelope / selector area */
#define AGX_DELTA_MAX_SIZE 50u       /* Replicator max-delta-size (reference.conf delta-crdt) */
#define AGX_DELTA_LOG_U32(orset) ((orset) ? 12u : 4u)
/* CRDT message rows (u32).  Full state: the data words, then (delta mode) deltaVersions[8].
 * DeltaPropagation (payload carries AGX_DELTA_ROW_BIT):
 *   [0] ops in the group (bit 31: NoDeltaPlaceholder) [1] from node [2] fromSeqNr [3] toSeqNr
 *   [4..11] the sender's deltaVersions, then the body --
 *   counters: [12] 1 = increments slot present | 2 = decrements slot present, [13..14] / [15..16] values;
 *   ORSet, per op: [type | n << 8] then AddDeltaOp: vvector(from), n x (element, version);
 *     RemoveDeltaOp: element, deltaDot version, vvector[8];  FullStateDeltaOp: vvector[8].
 * A group has < max-delta-size (<= 50) ops over <= AGX_DELTA_LOG seqNrs: <= 574 u32.  The row's
 * last word (pitch - 1) holds its used length in u32 (a queued row is copied forward that far). */
#define AGX_DELTA_ROW_BIT 0x20000000u
#define AGX_ORSET_DELTA_ROW_U32 576u
#define AGX_GCOUNTER_DELTA_WORDS (AGX_GCOUNTER_WORDS + AGX_DELTA_ENV_WORDS + AGX_COUNTER_DELTA_U32 / 2u)
#define AGX_PNCOUNTER_DELTA_WORDS (AGX_PNCOUNTER_WORDS + AGX_DELTA_ENV_WORDS + AGX_COUNTER_DELTA_U32 / 2u)
#define AGX_ORSET_DELTA_WORDS (AGX_ORSET_WORDS + AGX_DELTA_ENV_WORDS + AGX_DELTA_LOG * 6u)

/* --- LWWMap replicas (AGX_KIND_LWWMAP) -------------------------------------------------------
 * LWWMap[A, B] = ORMap[A, LWWRegister[B]] over the 64-key universe (DD/LWWMap.scala:144-150,175-187;
 * DD/ORMap.scala:254-265 put, :361-366 remove, :379-409 merge; DD/LWWRegister.scala:24-38 clocks,
 * :192-199 withValue / merge).  node = id % AGX_CRDT_NODES as for the other CRDT kinds.
 * State, AGX_LWWMAP_WORDS u64 per replica:
 *   w[0..259]              ORMap.keys: bit for bit the AGX_KIND_ORSET layout (64 keys x 8 u32 dots, the
 *                          8 u32 version vector)
 *   w[260 + k]             key k's LWWRegister.timestamp, an int64 in two's complement, compared signed
 *   u32 view, 648 + k      key k's (updatedBy node << 24) | value, value < 2^18   (w[324..355])
 * Canonical form: a key without a live dot has timestamp 0 and register word 0 (ORMap `values - key`);
 * every operation leaves this form, so states compare bit for bit.
 * Ops (control tells):
 *   AGX_OP_PUT     arg = key | value << 6   LWWMap.put(node, key, value, clock): timestamp' =
 *                  clock(timestamp) if the key is present, else clock(0); register = (node, value,
 *                  timestamp'); the key is added as AGX_OP_ADD adds an ORSet element (vvector + 1,
 *                  one birth dot).  (AGX_OP_PUT_ARG packs the argument: every 24-bit argument is a put.)
 *   AGX_OP_REMOVE  arg = key < 64           ORMap.remove: dots cleared as in the ORSet kind, register
 *                  cleared; key >= 64 is Behaviors.unhandled
 *   AGX_OP_GOSSIP  as for the other kinds; the state gossip's payload carries data type 3
 *   every other op (INCREMENT, DECREMENT, ADD, CLEAR, DELTA_TICK, unknown) is Behaviors.unhandled.
 * Merge of a received snapshot: the keys merge by ORSet.merge; a key of the merged set present on both
 * sides takes LWWRegister.merge (the higher timestamp wins, on a tie the lower node, else `this`
 * stays), a key present on one side takes that side's register, a key absent from the merged set has
 * its register cleared.
 * Clock (agx_set_lwwmap; logical time, so that runs are reproducible): now = base + s, where s is
 * the number of supersteps with mail the engine has run so far, the one that drains the put included
 * (agx_stats.supersteps at that superstep: 1 for the first superstep of a fresh engine).  A run
 * without mail executes no superstep with mail and does not advance s; the empty supersteps a
 * replayed batch may run after quiescence do not count either.
 *   AGX_LWW_CLOCK_DEFAULT  max(now, timestamp + 1)     LWWRegister.defaultClock
 *   AGX_LWW_CLOCK_REVERSE  min(-now, timestamp - 1)    LWWRegister.reverseClock (first write wins)
 * A timestamp that would pass the int64 range raises AGX_ERANGE (the reference's Long would wrap),
 * as a wrapping ORSet version does.
 * An LWWMap engine holds LWWMap replicas only, on one rank, with full-state gossip -- and, after
 * agx_set_lwwmap_delta, delta replication ("LWWMap delta replication" below).  Left out:
 * LWWRegister as a kind of its own, GSet, Flag, pruning, multi-rank engines,
 * custom clocks, the JVM shim.  (PNCounterMap and ORMultiMap are kinds of their own, below.)     */
#define AGX_LWWMAP_WORDS 356u /* 260 (keys) + 64 (timestamps) + 32 (64 u32 registers) */
#define AGX_LWWMAP_TS_WORD 260u
#define AGX_LWWMAP_REG_U32 648u
#define AGX_LWWMAP_VALUE_MAX 0x3FFFFu
#define AGX_OP_PUT 8u
#define AGX_OP_PUT_ARG(key, value) (((uint32_t)(key) & 63u) | ((uint32_t)(value) << 6))
#define AGX_LWW_CLOCK_DEFAULT 0u
#define AGX_LWW_CLOCK_REVERSE 1u

/* --- LWWMap delta replication (agx_set_lwwmap_delta; ORMap.DeltaOp, DD/ORMap.scala:30-164) -----
 * An LWWMap engine in this mode follows the delta contract of "delta-CRDT replication" above: keys
 * of AGX_CRDT_NODES consecutive replicas, the DeltaPropagationSelector (slice size, round robin,
 * deltaSentToNode), causal delivery (ORMap.DeltaOp is RequiresCausalDeliveryOfDeltas), full-state
 * gossip among the replicas of a key carrying the sender's deltaVersions.  LWWMap.put goes through
 * ORMap.put (DD/LWWMap.scala:144-150, DD/ORMap.scala:254-265), so the deltas are PutDeltaOp (the
 * ORSet.AddDeltaOp of the key and the full register) and RemoveDeltaOp only.
 * State, AGX_LWWMAP_DELTA_WORDS u64 per replica (u32 view):
 *   u32[0 .. 711]          the AGX_LWWMAP_WORDS data words, as above
 *   u32[712 + 0..7]        DataEnvelope.deltaVersions
 *   u32[712 + 8]           deltaCounter            u32[712 + 9]  deltaNodeRoundRobinCounter
 *   u32[712 + 10..17]      deltaSentToNode per node            (u32[712 + 18..23] always 0)
 *   u32[736 + 16 * (seq % AGX_DELTA_LOG) ..+ 15], a ring of AGX_DELTA_LOG entries of
 *   AGX_LWWMAP_DELTA_LOG_U32 u32, one per seqNr:
 *     PutDeltaOp     {seq, 1 | key << 8, the key's new dot version, register word, timestamp lo, hi, 0 x 10}
 *     RemoveDeltaOp  {seq, 2 | key << 8, 0 x 6, the remover's version vector[8]}   (DD/ORSet.scala:382)
 *   A local update that would overwrite a seqNr some node of the key has not been sent raises
 *   AGX_ECAPACITY, as for ORSet.
 * Local updates: every AGX_OP_PUT records one PutDeltaOp under the next seqNr, every AGX_OP_REMOVE
 * with key < 64 one RemoveDeltaOp (ORSet.add and ORSet.remove always yield a delta: no placeholder
 * comes from a local op).
 * AGX_OP_DELTA_TICK arg = k | AGX_DELTA_WRITE?: with AGX_DELTA_WRITE the replica first tells itself one
 * seeded update, r = fanout_rand(seed, self, k | 0x04000000, 0):
 *     ((r >> 40) & 3) != 0 ? AGX_OP_PUT, arg = AGX_OP_PUT_ARG((r >> 48) & 7, (r >> 8) & AGX_LWWMAP_VALUE_MAX)
 *                          : AGX_OP_REMOVE, arg = (r >> 48) & 7
 * then for each node of the slice with seqNrs after deltaSentToNode it folds those entries with
 * ORMap.DeltaOp.merge (DD/ORMap.scala:62-65,76-91,140-158): a put merges into the group's last op only
 * when that op is a put of the same key (the merged op keeps the later register and the later dot; the
 * merged one-node version vector is that dot, DD/ORSet.scala:57-76), everything else is appended.  A
 * group of two or more seqNrs with deltaSize (its ops) >= max_delta_size is a NoDeltaPlaceholder: not
 * told, deltaSentToNode advances all the same.  If k > 0, DELTA_TICK(k - 1) to itself.
 * DeltaPropagation row (payload data type 3 | AGX_DELTA_ROW_BIT), u32: the 12-u32 header of the other
 * delta kinds ([0] ops, [1] from node, [2] fromSeqNr, [3] toSeqNr, [4..11] the sender's deltaVersions),
 * then per op  PutDeltaOp {1 | key << 8, dot version, register word, timestamp lo, hi}  or
 * RemoveDeltaOp {2 | key << 8, version vector[8]}.  A group has at most AGX_DELTA_MAX_SIZE - 1 ops:
 * at most 12 + 9 * 49 = 453 u32 (AGX_LWWMAP_DELTA_ROW_U32); the row's last word (pitch - 1) holds
 * its used length.  A full-state row carries the 8 deltaVersions behind its data and counts them in
 * its length word: at most 736 + 8 u32 (AGX_LWWMAP_DELTA_STATE_ROW_U32), within the pitch of 768.
 * Receipt: skipped if toSeqNr <= deltaVersions(from) or fromSeqNr > deltaVersions(from) + 1; else
 * ORMap.mergeDelta (DD/ORMap.scala:425-503) -- dryMergeDelta walks the ops in order over a copy (a put:
 * keys.mergeDelta(AddDeltaOp), the value overwritten; a remove: the value dropped, mergeRemoveDelta),
 * then this.merge(copy) -- and deltaVersions(from) = toSeqNr.  The canonical form holds afterwards.
 * Left out: PNCounterMap and ORMultiMap deltas (UpdateDeltaOp, RemoveKeyDeltaOp, value deltas), mixed
 * populations, multi-rank engines, pruning, an unbounded delta log, the JVM shim.                   */
#define AGX_LWWMAP_DELTA_LOG_U32 16u
#define AGX_LWWMAP_DELTA_WORDS (AGX_LWWMAP_WORDS + AGX_DELTA_ENV_WORDS + AGX_DELTA_LOG * AGX_LWWMAP_DELTA_LOG_U32 / 2u) /* 880 */
#define AGX_LWWMAP_DELTA_ROW_U32 453u
#define AGX_LWWMAP_DELTA_STATE_ROW_U32 744u

/* --- PNCounterMap replicas (AGX_KIND_PNCOUNTERMAP) -------------------------------------------
 * PNCounterMap[A] = ORMap[A, PNCounter] over the 64-key universe (DD/PNCounterMap.scala:105-106 increment,
 * :139-141 decrement; DD/ORMap.scala:308-334 updated, :361-366 remove, :379-409 merge;
 * DD/PNCounter.scala:173-178 change, :180-183 merge).  node = id % AGX_CRDT_NODES as for the other CRDT kinds.
 * State, AGX_PNCMAP_WORDS u64 per replica (81 lines of 128 B):
 *   w[0..259]              ORMap.keys: bit for bit the AGX_KIND_ORSET layout (64 keys x 8 u32 dots, the
 *                          8 u32 version vector)
 *   w[260..271]            always 0 (padding: every key's counters start on a 128-B line)
 *   w[272 + 16k + n]       key k's increments of node n      (AGX_PNCMAP_CTR_WORD = 272)
 *   w[272 + 16k + 8 + n]   key k's decrements of node n
 * so each key's 16 words are an AGX_KIND_PNCOUNTER replica's 16 words; key k's value is the sum of its
 * increments less the sum of its decrements.
 * Canonical form: a key without a live dot has all 16 slots 0 (ORMap `values - key`); every operation
 * leaves this form, so states compare bit for bit.
 * Ops (control tells):
 *   AGX_OP_INCREMENT  arg = key | n << 6   PNCounterMap.increment(node, key, n), n < 2^18:
 *                     ORMap.updated(node, key, PNCounter())(_.increment(node, n)) -- the present counter,
 *                     or a fresh one, with node's increments slot raised by n (n = 0 leaves the counter as
 *                     it is, PNCounter.change); the key is added as AGX_OP_ADD adds an ORSet element
 *                     (vvector + 1, one birth dot), so an increment by 0 creates the key with value 0.
 *   AGX_OP_DECREMENT  arg = key | n << 6   PNCounterMap.decrement: likewise on node's decrements slot.
 *                     (AGX_OP_COUNT_ARG packs the argument: every 24-bit argument is valid.  A negative
 *                     delta cannot be expressed: decrement by n instead of incrementing by -n.)
 *   AGX_OP_REMOVE     arg = key < 64       ORMap.remove: dots cleared as in the ORSet kind, the 16 slots
 *                     cleared; key >= 64 is Behaviors.unhandled
 *   AGX_OP_GOSSIP     as for the other kinds; the state gossip's payload carries data type 3
 *                     (3 = the engine's ORMap-based map: a map engine holds one map kind only, so LWWMap
 *                     and PNCounterMap share the code)
 *   every other op (ADD, CLEAR, PUT, DELTA_TICK, unknown) is Behaviors.unhandled.
 * Merge of a received snapshot: the keys merge by ORSet.merge; a key of the merged set present on both
 * sides takes PNCounter.merge (the slot-wise maximum of all 16 slots), a key present on one side takes
 * that side's counter, a key absent from the merged set has its slots cleared.  As in the reference,
 * the values merge before it is known which dots survive: a key removed and counted again on one
 * replica gets its old slots back from a peer that still holds them.
 * AGX_ERANGE: a slot would pass 2^64 - 1 (the reference's BigInt would not wrap; as for
 * AGX_KIND_PNCOUNTER), or a replica's own version would pass 2^32 - 1 (as for ORSet and LWWMap).
 * A PNCounterMap engine holds PNCounterMap replicas only, on one rank, with full-state gossip and
 * n_words = AGX_PNCMAP_WORDS.  Left out: ORMap delta ops, pruning, multi-rank engines, mixed
 * populations, the JVM shim.  (ORMultiMap is a kind of its own, below.)                         */
#define AGX_PNCMAP_WORDS 1296u /* 260 (keys) + 12 (padding) + 64 * 16 (slots) = 81 lines of 128 B */
#define AGX_PNCMAP_CTR_WORD 272u
#define AGX_PNCMAP_COUNT_MAX 0x3FFFFu
#define AGX_OP_COUNT_ARG(key, n) (((uint32_t)(key) & 63u) | ((uint32_t)(n) << 6))

/* --- ORMultiMap replicas (AGX_KIND_ORMULTIMAP) -----------------------------------------------
 * ORMultiMap[A, B] = ORMap[A, ORSet[B]] over the 64-key universe, each key's set over a universe of
 * AGX_ORMM_VALUES = 8 values; the plain ORMultiMap.empty (withValueDeltas = false)
 * (DD/ORMultiMap.scala:78-91 merge, :182-189 put, :216-225 remove, :248-252 addBinding, :277-290
 * removeBinding, :310-318 replaceBinding; DD/ORMap.scala:308-334 updated, :361-366 remove, :379-409
 * dryMerge and merge; DD/ORSet.scala:339 add, :380 remove, :404 clear, :427- merge).
 * node = id % AGX_CRDT_NODES as for the other CRDT kinds.
 * State, AGX_ORMM_WORDS u64 per replica (161 lines of 128 B):
 *   w[0..259]              ORMap.keys: bit for bit the AGX_KIND_ORSET layout (64 keys x 8 u32 dots, the
 *                          8 u32 version vector)
 *   w[260..271]            always 0 (padding, as in a PNCounterMap replica)
 *   w[272 + 36k .. + 35]   key k's value ORSet[B] as 72 u32 (AGX_ORMM_SET_WORD = 272, AGX_ORMM_SET_U32 = 72):
 *                          u32 [0..7] the value set's own version vector, u32 [8 + 8v + n] the dot of
 *                          value v by node n, 0 = no dot.  Every block is 16-B aligned.
 * Canonical form: a key without a live key-dot has 72 zero u32 (ORMap `values - key`); every operation
 * leaves this form, so states compare bit for bit.  A live key may hold an empty set (put(key, Set())).
 * Ops (control tells):
 *   AGX_OP_ADD             arg = key | value << 6 < 512    addBinding(node, key, value):
 *                          ORMap.updated(node, key, ORSet.empty)(_.add(node, value)) -- the key is added as
 *                          AGX_OP_ADD adds an ORSet element (key-set vvector + 1, one birth dot); the
 *                          present set, or an empty one with a zero version vector, gets its own version
 *                          vector + 1 at node and the value's dots replaced by that one dot.
 *   AGX_OP_REMOVE_BINDING  arg = key | value << 6 < 512    removeBinding: the same `updated` with
 *                          ORSet.remove (the value's dots dropped, the set's version vector untouched); a
 *                          set left empty -- the value or the key may have been absent -- is followed by
 *                          ORMap.remove(node, key): key dots and the 72 u32 cleared, the key-set version
 *                          vector keeps the + 1.
 *   AGX_OP_PUT             arg = key | mask << 6, mask < 256 (bit v = value v)   put(node, key, set):
 *                          `updated` with clear() (all dots dropped, the version vector kept), then add of
 *                          every value of the mask in ascending value index.  (The reference folds over a
 *                          Scala Set in its iteration order; the order only decides which of the
 *                          consecutive versions each value gets, never `entries`.)  Mask 0 leaves a live
 *                          key with an empty set.
 *   AGX_OP_REPLACE_BINDING arg = key | old << 6 | new << 9 < 4096   replaceBinding: old == new returns
 *                          `this` (handled, no state change at all); otherwise addBinding(new) then
 *                          removeBinding(old) in one message.
 *   AGX_OP_REMOVE          arg = key < 64       remove(node, key) = ORMap.remove
 *   AGX_OP_GOSSIP          as for the other kinds; the state gossip's payload carries data type 3
 *   every other op, and every argument out of range, is Behaviors.unhandled.
 * Merge of a received snapshot: the keys merge by ORSet.merge; a key of the merged set present on both
 * sides takes ORSet.merge of the two value sets with their own version vectors, a key present on one
 * side takes that side's set, a key absent from the merged set has its 72 u32 cleared.  The reference's
 * anomalies are kept: a removeBinding concurrent with another node's addBinding to the same set can be
 * lost ("removals can be lost", ORMultiMap.scala:65), and a key removed and bound again starts a set with
 * a zero version vector, so it gets stale dots back from a peer that still holds the old set.
 * AGX_ERANGE: the key set's version or a value set's version at the node would pass 2^32 - 1.
 * An ORMultiMap engine holds ORMultiMap replicas only, on one rank, with full-state gossip and
 * n_words = AGX_ORMM_WORDS.  A snapshot row is up to 20 608 B: pass msg_capacity explicitly.  Left out:
 * ORMultiMap.emptyWithValueDeltas, ORMap delta ops, pruning, multi-rank engines, mixed populations, the
 * JVM shim.                                                                                      */
#define AGX_ORMM_VALUES 8u
#define AGX_ORMM_SET_U32 72u   /* 8 (version vector) + 8 values x 8 nodes */
#define AGX_ORMM_SET_WORD 272u
#define AGX_ORMM_WORDS 2576u /* 260 (keys) + 12 (padding) + 64 * 36 (value sets) = 161 lines of 128 B */
#define AGX_OP_REMOVE_BINDING 9u
#define AGX_OP_REPLACE_BINDING 10u
#define AGX_OP_BINDING_ARG(key, value) (((uint32_t)(key) & 63u) | (((uint32_t)(value) & 7u) << 6))
#define AGX_OP_PUT_SET_ARG(key, mask) (((uint32_t)(key) & 63u) | (((uint32_t)(mask) & 255u) << 6))
#define AGX_OP_REPLACE_ARG(key, old_value, new_value) \
  (((uint32_t)(key) & 63u) | (((uint32_t)(old_value) & 7u) << 6) | (((uint32_t)(new_value) & 7u) << 9))

typedef struct agx_cfg {
  uint32_t abi_version;   /* must be AGX_ABI_VERSION                                   */
  uint32_t device;        /* HIP device ordinal                                        */
  uint64_t n_actors;      /* global actor population (ids 0..n_actors-1), < 2^31       */
  uint32_t throughput;    /* dispatcher `throughput` (RC:541); <=0 behaves as 1 (Mailbox.scala:261) */
  uint32_t capacity;      /* bounded mailbox capacity C (Mailboxes.scala:212-216); 0 = unbounded */
  uint32_t n_words;       /* u64 state words: 1..AGX_MAX_GENERAL_WORDS, or AGX_MAX_WORDS */
  uint32_t max_emit;      /* max tells one message may emit (kmax)                     */
  uint32_t n_ranks;       /* GPUs the population is hash-sharded over (1 = single GPU) */
  uint32_t rank;          /* this engine's rank                                        */
  uint32_t num_shards;    /* ShardRegion number-of-shards (1000 in typed sharding)     */
  uint32_t bucket_actors;  /* actors per apply bucket: 0 = 2048, else a power of two in [32, 2048].
                             One workgroup drains a bucket; a bucket whose inbox exceeds 2048
                             messages takes the skew path -- populations with deep mailboxes
                             (ping-pong pairs, CRDT replicas with gossips) want small buckets */
  uint64_t msg_capacity;  /* max messages in flight on this rank (0 = 4 x local actors)*/
} agx_cfg;

typedef struct agx_stats {
  uint64_t delivered;     /* ActorCell.invoke calls (ActorCell.scala:539)              */
  uint64_t dead_letters;  /* overflow + to-stopped + to-unknown (Mailbox.scala:337-351,422-428) */
  uint64_t unhandled;     /* Behaviors.unhandled results (subset of delivered)         */
  uint64_t emitted;       /* tells emitted by behaviours                               */
  uint64_t staged;        /* tells staged from the host                                */
  uint64_t supersteps;    /* supersteps that had messages                              */
  uint64_t in_flight;     /* backlog + undelivered tells left when agx_run returned    */
  uint64_t bytes_alg;     /* algorithmic HBM bytes (SURVEY.md §8(d) formula)           */
} agx_stats;

typedef struct agx_engine agx_engine;

/* --- lifecycle ------------------------------------------------------------ */
agx_status agx_create(const agx_cfg* cfg, agx_engine** out);
agx_status agx_destroy(agx_engine* eng);
const char* agx_last_error(void);
uint32_t agx_abi_version(void);
/* 16 hex digits: the hash of the sources this library was built from (a build check, no
 * reference counterpart; __graft_entry__.source_hash computes the same over csrc/ and this header) */
const char* agx_build_hash(void);

/* --- actor registration (actorOf for a contiguous id range) --------------- */
/* init_state: count x state_stride bytes, actor-major, n_words u64 used per actor
 * (may be NULL = zero state).  Only ids owned by this rank are kept.         */
agx_status agx_register_range(agx_engine* eng, uint64_t first_id, uint64_t count,
                              uint32_t kind, const void* init_state, size_t state_stride);

/* --- behaviour parameters --------------------------------------------------- */
agx_status agx_set_ring(agx_engine* eng, uint32_t stride);
/* Zipf targets: cdf[i] = ceil(2^32 * P(rank <= i)) - 1 style u32 thresholds
 * (non-decreasing, cdf[n-1] = 0xFFFFFFFF); perm maps rank -> actor id.      */
agx_status agx_set_fanout(agx_engine* eng, uint32_t k, uint64_t seed, const uint32_t* cdf,
                          const uint32_t* perm, uint64_t n);
/* CRDT gossip: each GOSSIP tick sends the replica's state to `fanout` peers
 * drawn uniformly from the other actors with the counter RNG (seed, self,
 * countdown, j) — Replicator.selectRandomNode (DD/Replicator.scala:2063-2064). */
agx_status agx_set_gossip(agx_engine* eng, uint32_t fanout, uint64_t seed);
/* Delta-CRDT replication (Replicator `delta-crdt.enabled = on`, `max-delta-size`,
 * akka-distributed-data/src/main/resources/reference.conf:65-72): 0 = off (full-state
 * gossip among all replicas of one key), 1..AGX_DELTA_MAX_SIZE = on, with keys of 8 replicas
 * (see "delta-CRDT replication" above).  Call before the first agx_run; CRDT actors then need
 * n_words >= the *_DELTA_WORDS of their kind.                                               */
agx_status agx_set_delta_crdt(agx_engine* eng, uint32_t max_delta_size);
/* The LWWRegister clock of an LWWMap engine (see "LWWMap replicas" above): clock =
 * AGX_LWW_CLOCK_DEFAULT / AGX_LWW_CLOCK_REVERSE, base < 2^62.  Optional (default clock, base 0);
 * call after registering the LWWMap replicas and before the first agx_run (AGX_ESTATE afterwards).
 * AGX_EINVAL: an engine without LWWMap replicas, an unknown clock, base >= 2^62.                  */
agx_status agx_set_lwwmap(agx_engine* eng, uint32_t clock, uint64_t base);
/* Delta replication for an LWWMap engine (see "LWWMap delta replication" above): max_delta_size =
 * 1..AGX_DELTA_MAX_SIZE.  Call after registering the LWWMap replicas and before the first agx_run
 * (AGX_ESTATE afterwards); agx_set_lwwmap keeps working, in either order.  AGX_EINVAL: an engine without
 * LWWMap replicas, max_delta_size out of range, max_emit < 4, more than one rank, n_words <
 * AGX_LWWMAP_DELTA_WORDS.  (agx_set_delta_crdt stays refused on an LWWMap engine.)                  */
agx_status agx_set_lwwmap_delta(agx_engine* eng, uint32_t max_delta_size);
/* Compiled behaviours (see "compiled behaviours" above): behaviour b = cases
 * [first[b], first[b+1]); first has n_behaviors + 1 entries.  Replaces the tables of an
 * earlier call; call before agx_run.  Register actors with kind AGX_KIND_COMPILED + b.      */
agx_status agx_set_behaviors(agx_engine* eng, const agx_case* cases, uint32_t n_cases, const agx_act* acts,
                             uint32_t n_acts, const uint32_t* first, uint32_t n_behaviors);
/* Out-edge lists in CSR over GLOBAL ids: row_ptr[n_actors+1], col[row_ptr[n]].  */
agx_status agx_set_graph(agx_engine* eng, const uint64_t* row_ptr, const uint32_t* col);
/* The same CSR with the destinations generated on the device (workload setup for
 * 10^8-actor graphs; not part of the dispatcher boundary): edge e gets the R-MAT
 * destination of `bits` quadrant draws q = splitmix64(e*64 + bit + seed) & 0xFFFF,
 * destination bit = (ta <= q < tb) | (q >= tc), reduced mod n_actors.          */
agx_status agx_set_graph_rmat(agx_engine* eng, const uint64_t* row_ptr, uint32_t bits, uint32_t ta,
                              uint32_t tb, uint32_t tc, uint64_t seed);

/* --- tell / run ------------------------------------------------------------- */
/* Host tells (caller-owned buffers, copied).  src may be AGX_NO_SENDER.
 * Tells whose dst is not owned by this rank are ignored on this rank.
 * All or nothing: AGX_EINVAL (a tagged sender) or AGX_ECAPACITY (the tells would take the
 * messages in flight on this rank past msg_capacity) stages none of them and leaves every
 * counter unchanged -- run the engine to drain it and stage again.                              */
agx_status agx_stage_tells(agx_engine* eng, const uint32_t* dst, const uint32_t* src,
                           const uint32_t* payload, size_t n);
/* The lock-free tell path (ActorRef.! from any thread; the reference: one getAndSet enqueue,
 * akka-actor/src/main/java/akka/dispatch/AbstractNodeQueue.java:79-82, and a CAS-guarded schedule,
 * akka-actor/src/main/scala/akka/dispatch/Mailbox.scala:185-194 + Dispatcher.scala:120-128).
 * agx_tell may be called from any number of threads at once, also while one thread is inside
 * agx_run: each calling thread appends to a queue of its own (wait-free, each sender's tells in
 * order; the next agx_run takes them as agx_stage_tells would).  *schedule = 1 iff this tell moved
 * the engine from idle to scheduled: the caller then submits ONE pump task (a task that calls
 * agx_run and then agx_pump_idle); N tells to an idle engine submit one.  agx_pump_idle is the
 * pump's last call (Mailbox.run's finally: setAsIdle, then registerForExecution if the mailbox
 * still has messages, Mailbox.scala:227-240): *reschedule = 1 iff tells arrived after the pump's
 * last agx_run, or tells are still queued because they did not fit the message capacity, or the
 * last agx_run succeeded and left mail in flight (a superstep budget) -- submit the pump again.
 * Tells are never refused or lost at capacity: agx_run takes only as many queued tells as fit
 * msg_capacity beside the mail already in flight, the rest wait in the queue for a later pump
 * (back-pressure, as an unbounded MPSC mailbox never refuses an enqueue, AbstractNodeQueue.java:
 * 79-82; a bounded mailbox class still tail-drops at its own capacity).  agx_pump_cancel: the pump
 * could not be submitted (the executor rejected it): the engine goes back to idle without the
 * re-check, so the next tell schedules it again (Dispatcher.registerForExecution's catch,
 * Dispatcher.scala:130-138).  (src may be AGX_NO_SENDER; schedule / reschedule may be NULL.)  */
agx_status agx_tell(agx_engine* eng, uint32_t dst, uint32_t src, uint32_t payload, int32_t* schedule);
agx_status agx_pump_idle(agx_engine* eng, int32_t* reschedule);
agx_status agx_pump_cancel(agx_engine* eng);
/* Run up to max_supersteps supersteps or until quiescent; stats are cumulative
 * over the engine's lifetime.  On an engine with timers (agx_set_timers) a superstep is a tick, a
 * tick without mail still counts against max_supersteps, and quiescent means no mail in flight and
 * no timer pending: a periodic timer never lets the engine go quiescent, so agx_run on such an
 * engine is always given a budget.  out may be NULL: the counters are then not read
 * back (agx_get_stats does it later, and reports AGX_ECAPACITY if an overflow
 * was recorded meanwhile).                                                    */
agx_status agx_run(agx_engine* eng, uint32_t max_supersteps, agx_stats* out);
agx_status agx_get_stats(agx_engine* eng, agx_stats* out);
/* agx_run, plus the run's device time in ms: HIP events on the engine's stream before the first
 * launch and after the last superstep (bench.py's roofline timing of graph-replayed supersteps). */
agx_status agx_run_timed(agx_engine* eng, uint32_t max_supersteps, agx_stats* out, float* device_ms);
/* Supersteps of a single-rank multi-pass engine (> 2^20 actors) whose mail needed no radix pass:
 * the previous apply's tells were already in destination order (a ring, a stencil -- identity
 * grouping).  Diagnostic; the grouping is the same either way.                  */
agx_status agx_identity_supersteps(agx_engine* eng, uint64_t* out);
/* Bounded-mailbox ring slots handed out so far (high-water mark; single-rank multi-pass engine whose
 * mailbox classes are all bounded): a bucket that holds more than one LDS tile of
 * mail keeps its actors' queued messages in per-actor rings of the largest capacity -- a queued
 * message is written once and read once -- until its rings are empty and its mail fits one tile
 * again (the slot is then reused).  Diagnostic; the semantics are the same either way. */
agx_status agx_ring_buckets(agx_engine* eng, uint64_t* out);
/* Multi-rank exchange accounting of this rank (diagnostic): out[0] supersteps on the device-resident
 * exchange (fixed per-peer slabs), out[1] supersteps on the host-planned exchange (exact per-peer
 * sizes), out[2] envelope bytes and out[3] CRDT row bytes sent to peers, out[4] 1 once the CRDT row
 * slabs did not fit on some rank (row handle space, AGX_MR_ROW_MB or memory) and every rank moved to
 * the host-planned exchange, out[5] the slab (envelopes per peer per superstep). */
agx_status agx_exchange_info(agx_engine* eng, uint64_t out[6]);
/* Persistent fused supersteps (diagnostic): out[0] replays launched as ONE persistent
 * launch (a strict replay whose supersteps are the dense launch alone: k_dense_fused runs them with a
 * grid barrier between supersteps; opt-in: AGX_PERSIST=1), out[1] supersteps they ran. */
agx_status agx_persist_info(agx_engine* eng, uint64_t out[2]);

/* --- per-actor mailboxes (Mailboxes.lookupConfigurator, Mailboxes.scala:204-260) -------------
 * An actor's mailbox type is resolved per actor in the reference (props, then dispatcher, then
 * requirement; ActorMailboxSpec.scala:245-450).  Here a dispatcher's actors use one of
 * AGX_MAX_MAILBOX_CLASSES mailbox classes: class 0 is agx_cfg.capacity, classes 1..7 are set by
 * agx_set_mailbox_class (bounded-capacity:N -> N; an unbounded mailbox type -> 0), and
 * agx_set_mailbox binds a range of actors to a class (default: class 0).  A bounded class drains at
 * most min(throughput, capacity) messages per mailbox run, as a bounded queue never holds more.    */
#define AGX_MAX_MAILBOX_CLASSES 8u
agx_status agx_set_mailbox_class(agx_engine* eng, uint32_t mailbox_class, uint32_t capacity);
agx_status agx_set_mailbox(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t mailbox_class);
/* Mailbox.scala:726-816 (priority / stable priority), :867-1025 (control-aware)
 * A mailbox class may carry a priority table: the priority of a message is prio[payload >> 24] (the
 * message tag), a lower value is dequeued first (PriorityGenerator's comparator), equal priorities stay
 * in arrival order across supersteps (StablePriorityBlockingQueue's (priority, sequence number)).
 * Admission is unchanged and goes by arrival position (a bounded priority queue's offer fails when
 * the queue is full, whatever the priority: Mailbox.scala:761-766, 810-815); the admitted messages
 * of an actor are then stably sorted by priority, the first min(len, throughput) are drained and
 * the rest is the backlog, kept in that order.  A control-aware mailbox is the
 * table 0 for control tags, 1 for all others.  prio == NULL clears the class's table; a class
 * without a table is FIFO.  The class must be configured (class 0 always is); call before the first
 * agx_run (AGX_ESTATE afterwards).  AGX_EINVAL: an engine with n_ranks > 1, an engine with a CRDT
 * kind registered (a snapshot handle has no tag; registering one after this call is refused the
 * same way), an unconfigured class, an engine whose bounded-mailbox ring pool exists.
 * The one bounded difference from the reference: a prioritised actor's whole queue must be seen
 * by one workgroup, so a bucket (agx_cfg.bucket_actors actors) that holds an actor of a prioritised
 * class and whose inbox -- backlog included -- exceeds one 2048-message tile makes agx_run return
 * AGX_ECAPACITY (sticky; never a silently wrong order).  Buckets without such an actor are not
 * limited. */
agx_status agx_set_mailbox_priority(agx_engine* eng, uint32_t mailbox_class, const uint8_t prio[256]);
/* Deque-based mailboxes and the stash (Unbounded/BoundedDequeBasedMailbox, Mailbox.scala; classic
 * Stash.scala `stash-capacity`; typed StashBuffer, TY/internal/StashBufferImpl.scala:61-79,131-218).
 * A mailbox class with a stash capacity S (1..255) gives each of its actors a stash buffer of at most
 * S envelopes outside its mailbox: it never counts towards the mailbox capacity.  A compiled case with
 * result AGX_RES_STASH appends the message to the buffer (sender and payload kept; not counted
 * delivered; a full buffer stops the actor, StashOverflowException under typed's default supervision);
 * AGX_RES_UNSTASH_ALL releases what the buffer holds at that point: the drain ends there, and the
 * following supersteps process the released messages, up to `throughput` each, before any mailbox
 * message (mail that arrives meanwhile is queued; the unprocessed rest of that drain is parked and
 * comes next).  Messages stashed while released ones are processed go behind them and stay held
 * (DESIGN.md 2.2).  A stopping actor's buffered and parked messages are dead letters.  Held messages
 * do not keep agx_run going; agx_stats.in_flight includes every buffered and parked message.
 * The class must be configured; call before the first agx_run (AGX_ESTATE afterwards).  AGX_EINVAL:
 * capacity 0 or above 255 (there is no unbounded stash: stash-capacity = -1 is not supported), an
 * engine with n_ranks > 1, with a CRDT kind or a priority table (either call order), with max_emit
 * above 1, an unconfigured class, an engine whose bounded-mailbox ring pool exists.  AGX_ENOMEM: the
 * per-actor buffers (n_actors x (largest S + throughput - 1) envelopes) do not fit.
 * The one bounded difference from the reference: a bucket (agx_cfg.bucket_actors actors) that holds an
 * actor of such a class and whose inbox -- backlog and the released messages due this superstep
 * included -- exceeds one 2048-message tile makes agx_run return AGX_ECAPACITY (sticky).  Buckets
 * without such an actor are not limited. */
agx_status agx_set_stash(agx_engine* eng, uint32_t mailbox_class, uint32_t capacity);
/* Totals since agx_create: messages stashed, released by unstash_all, StashOverflowExceptions; and
 * right now: buffered messages not released (held), released or parked messages still to be
 * processed (pending).  Any pointer may be NULL. */
agx_status agx_stash_info(agx_engine* eng, uint64_t* stashed, uint64_t* unstashed, uint64_t* overflows,
                          uint64_t* held, uint64_t* pending);
/* One actor's stash buffer in order (for tests and tools): up to `cap` envelopes into src / payload,
 * *n = the buffer's size, *n_released = how many of its first entries are released. */
agx_status agx_read_stash(agx_engine* eng, uint64_t actor_id, uint32_t* src, uint32_t* payload, uint32_t cap,
                          uint32_t* n_released, uint32_t* n);
/* The behaviour kind of actors [first_id, first_id + count) now, one byte each: a compiled behaviour's become
 * and unstash_all(next) change it (AGX_KIND_COMPILED + behaviour).  Single-rank engines (for tests and tools). */
agx_status agx_read_kinds(agx_engine* eng, uint64_t first_id, uint64_t count, uint8_t* kinds);
/* Compiled tables with a stash / unstash_all result on an engine without any stash class make agx_run
 * return AGX_EINVAL.  On an engine with one, an actor of a class without a capacity that runs a stash
 * case overflows and stops -- except in a bucket without any actor of a stash class whose inbox exceeds
 * one tile: that bucket takes the skew launch, which does not interpret the stash results (the message
 * is handled as Behaviors.same); keep such actors off behaviours that stash. */

/* Timers (Behaviors.withTimers / TimerScheduler, TY/internal/TimerSchedulerImpl.scala:61-172; the classic
 * dungeon/TimerSchedulerImpl.scala has the same rule; DESIGN.md 2.3 has the contract).
 * Logical time: one superstep is one tick, a delay is a count of ticks >= 1 -- the reference's scheduler
 * under manual time.  The scheduled task is only `self ! timerMsg`, so startTimerWithFixedDelay and
 * startTimerAtFixedRate coincide (both fire at start + d, start + 2d, ...): one periodic op.
 * agx_set_timers gives every actor n_keys (1..4) timer slots; the key is the slot index.  A slot is
 * active or not and holds the tick of its next fire (or none to come), the period (0: single), a
 * generation and the message payload; an actor's generation counter starts at 1 (timerGen).  Starting
 * key k at tick s with delay d cancels the slot if active, gives it the actor's next generation and a
 * next fire at s + d.  At tick s every alive actor's active slot whose next fire is s sends a TimerMsg
 * to the actor's own mailbox: sender = the actor, payload = AGX_TAG_TIMER << 24 | key << 22 |
 * (generation mod 2^22).  It comes last in that tick's inbox -- after the backlog, the arrivals and the
 * host-staged tells, in key order -- and is admitted by position like any message (in a full bounded
 * mailbox it is a dead letter; a single timer whose message died stays active and never fires again,
 * as in the reference).  A periodic slot's next fire becomes s + period, a single slot's none to come.
 * Receipt (interceptTimerMsg): a drained message with tag AGX_TAG_TIMER takes a drain slot and counts
 * as delivered; if slot `key` is inactive or its generation differs (compared mod 2^22) it is discarded
 * -- the behaviour does not run, `discarded` grows, it is not unhandled -- else a single slot becomes
 * inactive and the behaviour runs on the slot's stored payload with sender = the actor itself.
 * Cancelling leaves an already enqueued message in the mailbox (it is discarded at receipt); a stopping
 * actor's slots all become inactive; a become leaves them alone.
 * Tag AGX_TAG_TIMER is reserved: agx_stage_tells / agx_tell refuse it (AGX_EINVAL); a payload a
 * behaviour computes that lands on it is taken for a TimerMsg (and normally discarded).
 * Conservation: staged + emitted + fired = delivered + dead_letters + in_flight.
 * Call before the first agx_run (AGX_ESTATE afterwards).  AGX_EINVAL: n_keys outside 1..4, n_ranks > 1,
 * an engine with a CRDT kind, a priority table or a stash class (either call order), an engine whose
 * bounded-mailbox ring pool exists, max_emit > 1 (a timer action must take effect once).  AGX_ENOMEM: the
 * slots do not fit.  An engine with timers uses no wave, ring, dense or persistent launch, and a bucket
 * (agx_cfg.bucket_actors actors) whose inbox -- backlog and the tick's TimerMsgs included -- exceeds one
 * 2048-message tile makes agx_run return AGX_ECAPACITY (sticky).  Tables with a timer action or
 * AGX_V_TIMER on an engine without timers (or with a key >= n_keys) make agx_run return AGX_EINVAL. */
agx_status agx_set_timers(agx_engine* eng, uint32_t n_keys);
/* withTimers' setup block: start timer `key` of actors [first_id, first_id + count) at the current tick
 * (before the first run or between runs), single or periodic, with message payload `payload`.  The first
 * fire comes after `delay` ticks -- or after delays[i] ticks for actor first_id + i when `delays` is not
 * NULL (staggered phases); a periodic timer's period is `delay` either way.  A delay of 0 counts as 1, one
 * above 2^31 - 1 is clamped.  Stopped actors are skipped.  AGX_EINVAL on an engine without timers (and the
 * engine's agx_run then returns AGX_EINVAL too), or for a key >= n_keys. */
agx_status agx_start_timers(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t key, int32_t periodic,
                            uint32_t delay, const uint32_t* delays, uint32_t payload);
/* Totals since agx_create: TimerMsgs sent (those that died at admission included), TimerMsgs discarded
 * at receipt; right now: active slots, pending slots (active with a fire still to come: every active
 * periodic slot, an active single slot that has not fired); and ticks: the supersteps that ran while
 * the engine was not quiescent (agx_stats.supersteps still counts only those with mail).  Any pointer
 * may be NULL. */
agx_status agx_timer_info(agx_engine* eng, uint64_t* fired, uint64_t* discarded, uint64_t* active, uint64_t* pending,
                          uint64_t* ticks);
/* One actor's timer slots (for tests and tools): remaining = ticks to the next fire, 0xFFFFFFFF when
 * none is to come.  Slots past n_keys read as zero (remaining 0xFFFFFFFF).  Any pointer may be NULL. */
agx_status agx_read_timers(agx_engine* eng, uint64_t actor_id, uint32_t active[4], uint32_t remaining[4],
                           uint32_t period[4], uint32_t payload[4], uint32_t generation[4]);

/* Receive timeouts (context.setReceiveTimeout / cancelReceiveTimeout: AA/dungeon/ReceiveTimeout.scala:18-74, typed
 * TY/internal/adapter/ActorContextAdapter.scala:120-131, ActorAdapter.scala:92-93; pinned by ReceiveTimeoutSpec.scala:
 * 63-278 and ActorContextSpec.scala:565-610; DESIGN.md 2.7 has the contract).  On top of the timers: call
 * agx_set_timers first; time is the timers' logical time.
 * Every actor has a delay (ticks, 0: no timeout set), a message payload and a next fire (a tick, or none to come).
 * AGX_A_SET_RECEIVE_TIMEOUT(d, msg) in a case run at tick s stores (d, msg) with next fire s + d, whatever the
 * handled message is; AGX_A_CANCEL_RECEIVE_TIMEOUT sets delay 0 and none to come (an envelope already enqueued stays
 * in the mailbox); any stop turns the timeout off, a become leaves it alone.
 * Influence: every drained message whose tag is not transparent, drained at tick s by an actor with a timeout set
 * (after its case ran, handled or not), moves the next fire to s + delay.  The tag is that of the payload the
 * behaviour sees (an accepted TimerMsg: the slot's stored payload); the receive-timeout message itself influences;
 * a transparent message that neither sets nor cancels leaves the next fire as it is, none to come included; queued
 * messages left in the backlog, dead letters, discarded TimerMsgs and discarded envelopes do not influence.
 * `transparent_tags` is a 256-bit mask over message tags (bit t of word t / 32: tag t is
 * NotInfluenceReceiveTimeout); NULL: none.
 * Fire: at tick s every alive actor with a timeout set and next fire s sends one envelope to its own mailbox:
 * sender = the actor, payload = AGX_TAG_RECEIVE_TIMEOUT << 24, last in that tick's inbox (after the tick's TimerMsgs),
 * admitted by position (a dead letter in a full bounded mailbox; the next processed message reschedules).  The next
 * fire becomes none to come: the reference's task is one-shot and the next influencing receipt, normally the
 * envelope's own, reschedules it -- an idle actor gets the message every d ticks until it cancels or stops.
 * Receipt: a drained envelope takes a drain slot and counts as delivered.  With a timeout set at that point of the
 * window the behaviour runs on the message stored now (there is no generation: a stale envelope is delivered with the
 * replaced message, as in the reference) with sender = the actor, and influences; with none set it is discarded
 * (`discarded`, not unhandled; the typed reference would hand the behaviour null here).
 * Tag AGX_TAG_RECEIVE_TIMEOUT is reserved on such an engine as AGX_TAG_TIMER is: agx_stage_tells, agx_tell,
 * agx_start_timers payloads and tables naming it are refused; a computed payload landing on it is taken for the envelope.
 * Conservation: staged + emitted + timer fired + receive-timeout fired = delivered + dead_letters + in_flight.
 * A pending receive timeout keeps the engine non-quiescent and agx_pump_idle rescheduling, as a pending timer does.
 * AGX_EINVAL without timers ("receive timeouts need an engine with timers"), on a second call, or when tables, staged
 * tells or recorded timer starts name the reserved tag; AGX_ESTATE after the first run; AGX_ENOMEM: the rows do not
 * fit.  agx_set_timers cannot change the key count afterwards.  Tables that hold either action, or
 * agx_start_receive_timeout, on an engine without receive timeouts make agx_run return AGX_EINVAL. */
agx_status agx_set_receive_timeout(agx_engine* eng, const uint32_t transparent_tags[8]);
/* The setup block: every live actor of [first_id, first_id + count) sets (delay, payload) at the current tick (before
 * the first run or between runs); delay 0 cancels; a delay above 2^31 - 1 is clamped. */
agx_status agx_start_receive_timeout(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t delay, uint32_t payload);
/* Totals since agx_create: envelopes sent (those that died at admission included), envelopes discarded at receipt;
 * right now: actors with a timeout set, and those of them with a fire still to come.  agx_timer_info keeps counting
 * timer slots only.  Any pointer may be NULL. */
agx_status agx_receive_timeout_info(agx_engine* eng, uint64_t* fired, uint64_t* discarded, uint64_t* set, uint64_t* pending);
/* The timeouts of actors [first_id, first_id + count) (for tests and tools): remaining = ticks to the next fire,
 * 0xFFFFFFFF when none is to come.  Any pointer may be NULL. */
agx_status agx_read_receive_timeout(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t* delay, uint32_t* remaining,
                                    uint32_t* payload);

/* Sharded entities (akka-cluster-sharding Shard.scala: getOrCreateEntity :504-516, passivate :405-417, deliverMessage /
 * appendToMessageBuffer :469-496, entityTerminated / passivateCompleted / sendMsgBuffer :388-400, :437-466; DESIGN.md
 * 2.13 has the contract).  On top of receive timeouts: call agx_set_timers and agx_set_receive_timeout first; time is
 * the timers' logical time.  An entity type is a range of unregistered ids [first_id, first_id + count) in [0,
 * n_actors), pairwise disjoint, with a compiled behaviour `kind`, the state a start gives (word 0 = base0, word 1 =
 * `word1` or, with AGX_ENTITY_WORD1_ID, the entity's id; other words 0), the stop message payload, and the receive
 * timeout (idle_delay ticks, idle_payload) a start sets -- idle_delay 0: none.
 * Start: at the inbox formation of tick t a not-alive entity with at least one starting item -- an item whose sender
 * is not the entity itself -- becomes alive before admission with its type's kind and state and, with an idle delay,
 * the receive timeout set at tick t; `started` and the id's incarnation count grow; the tick's mail is admitted as for
 * any live actor.  Items the entity sent itself (a self-tell, a TimerMsg, a receive-timeout envelope) never start it:
 * to a stopped entity they are dead letters at that formation.
 * A stop without Passivate is today's stop: timers and timeout off, the rest of the window and the queued mail are
 * dead letters (the queued mail at the next formation); mail of a later tick starts a new incarnation.
 * AGX_A_PASSIVATE run at tick s by an entity that is not passivating marks it, sends the type's stop payload to the
 * entity itself (sender = the entity; `emitted`; it arrives with tick s + 1's arrivals) and counts `passivations`; run
 * by a passivating entity nothing is sent (`passivate_ignored`), by an actor in no entity range the same
 * (`passivate_unknown`).  A stop while passivating counts `passivated`: everything queued behind the stop -- the rest
 * of the tick's admitted inbox, later arrivals -- stays queued and is no dead letter, except what the entity sent
 * itself, which dies at the next formation.  If anything stays the entity starts again at the formation of the next
 * tick (`restarted` as well as `started`) and receives that mail in order.  Any stop clears the mark.
 * Bounded differences: an entity that handles its stop message without stopping goes on receiving; the buffer's bound
 * is the entity's mailbox capacity with tail-drop; a stale receive-timeout envelope can reach a new incarnation.
 * Conservation is that of receive timeouts.  A passivating entity with queued mail keeps the engine non-quiescent.
 * AGX_EINVAL: without receive timeouts ("sharding needs an engine with receive timeouts"), on a second call, with the
 * ask pattern, for n_types outside 1..AGX_MAX_ENTITY_TYPES, a type that is empty, leaves [0, n_actors), overlaps
 * another, holds a registered id, names a kind that is no compiled behaviour kind, unknown flags, or a stop or idle
 * payload with a reserved tag (0xFF, 0xFB); AGX_ESTATE after the first run; AGX_ENOMEM.  agx_register_range into an
 * entity range is AGX_EINVAL in either call order.  Tables that hold AGX_A_PASSIVATE on an engine without sharding
 * make agx_run return AGX_EINVAL; a case with PASSIVATE beside a TELL is refused by agx_set_behaviors. */
typedef struct agx_entity_type {
  uint32_t first_id, count;
  uint32_t kind;          /* AGX_KIND_COMPILED + b */
  uint32_t flags;         /* AGX_ENTITY_WORD1_ID or 0 */
  uint64_t base0, word1;  /* state words 0 and 1 of a start */
  uint32_t stop_payload;  /* the stop message AGX_A_PASSIVATE sends */
  uint32_t idle_delay, idle_payload;  /* the receive timeout a start sets (idle_delay 0: none) */
  uint32_t reserved;      /* 0 */
} agx_entity_type;
agx_status agx_set_sharding(agx_engine* eng, const agx_entity_type* types, uint32_t n_types);
/* Totals since agx_create: started, restarted, passivations, passivated, passivate_ignored, passivate_unknown; right
 * now: the entities alive.  Any pointer may be NULL. */
agx_status agx_sharding_info(agx_engine* eng, uint64_t* started, uint64_t* restarted, uint64_t* passivations,
                             uint64_t* passivated, uint64_t* passivate_ignored, uint64_t* passivate_unknown,
                             uint64_t* alive);
/* The ids [first_id, first_id + count) (for tests and tools): alive, the incarnation count, passivating.  Ids in no
 * entity range read 0 incarnations.  Any pointer may be NULL. */
agx_status agx_read_entities(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t* alive, uint32_t* incarnations,
                             uint32_t* passivating);

/* The ask pattern: request-response with a timeout (ActorContext.ask: TY/internal/ActorContextImpl.scala:203-218;
 * AskPattern.ask: TY/scaladsl/AskPattern.scala:109-162; pinned by ActorContextAskSpec.scala:41-189 and AskSpec.scala:
 * 64-110; DESIGN.md 2.9 has the contract).  On top of the timers: call agx_set_timers first; time is the timers'.
 * An ask uses one of the actor's timer keys, so an actor has at most n_keys asks outstanding.
 * AGX_A_ASK_ARM(k, t, m, a) + AGX_A_ASK_SEND(k, d, p) in a case run at tick s: key k is started as a single timer
 * (the previous occupant is cancelled, the slot gets the actor's next generation g, next fire s + t, stored payload
 * m) and marked as an ask with adapt tag a or none; one envelope (d, p) is emitted whose sender field is the ask
 * ref AGX_ASK_REF_BIT | k << 29 | (g mod 2^7) << 22 | the actor's id.  The target sees the ref as the sender and may
 * keep it in a state word.
 * Answering: every tell emitted on such an engine, by whichever kind, whose destination has bit 31 set and is not
 * 0xFFFFFFFF is a reply: it is emitted to the ref's id with the ref as the sender field (the replier's id is not
 * carried).  Receipt: a drained envelope whose sender field is a ref that names the receiving actor is a reply (an
 * actor that asks itself gets its request as the reply).  It takes a drain slot and counts as delivered.  Slot k
 * active, an ask, and of the ref's generation mod 2^7: the slot becomes inactive as a cancel makes it, the behaviour
 * runs with sender = the actor on (payload & 0xFFFFFF) | a << 24, or on the payload unchanged without an adapt tag.
 * Otherwise the reply is late: counted, discarded, not unhandled.  The timeout is the slot's TimerMsg: accepted, the
 * behaviour runs on m with sender = the actor.  The inbox order is the timers': a reply that arrives in the tick of
 * the fire wins.  A round trip takes two ticks, so t = 1 always times out.
 * Cancelling the key abandons the ask; a stop of the asker cancels its slots; AGX_V_TIMER on the key reads "ask
 * outstanding".  Conservation and quiescence are the timers': the request counts as emitted, the timeout as fired,
 * and an outstanding ask is a pending single timer.
 * AGX_EINVAL without timers, on a second call, together with receive timeouts (either order) or with more than
 * AGX_ASK_MAX_ACTORS actors; AGX_ESTATE after the first run; AGX_ENOMEM: the row does not fit.  agx_set_timers cannot
 * change the key count afterwards.  Tables that hold an ask action on an engine without ask, an ASK_SEND not directly
 * preceded by the ASK_ARM of its key, or an ask key >= n_keys make agx_run return AGX_EINVAL. */
agx_status agx_set_ask(agx_engine* eng);
/* Totals since agx_create: asks made, replies accepted, timeouts delivered, late replies discarded.  Any pointer may
 * be NULL. */
agx_status agx_ask_info(agx_engine* eng, uint64_t* asked, uint64_t* answered, uint64_t* timed_out, uint64_t* late);
/* The ask marks of an actor's timer slots (for tests and tools): is_ask[k] = 1 when slot k is active as an ask's
 * timeout, adapt[k] = its adapt tag, 0xFFFFFFFF without one or when the slot is no ask.  Any pointer may be NULL. */
agx_status agx_read_asks(agx_engine* eng, uint64_t actor_id, uint32_t is_ask[4], uint32_t adapt[4]);

/* Death watch (context.watch / watchWith / unwatch and the Terminated signal: AA/dungeon/DeathWatch.scala:19-113,
 * :147-162; typed adapter TY/internal/adapter/ActorAdapter.scala:84-91,134-138,200-205; pinned by
 * WatchSpec.scala:54-85,196-362; DESIGN.md 2.4 has the contract).
 * agx_set_death_watch gives every actor n_slots (1..4) watch slots.  Time is the timers' logical time: one
 * superstep is one tick.  Every actor has a death tick, "none" while alive, set to the tick in which it stops;
 * an id that was never registered counts as dead before tick 1, and so does any id outside [0, n_actors)
 * (host-side actors cannot be watched in this version).
 * A slot is free, watching, due or notified and holds the watchee, an optional custom message, and a
 * generation (+1 at every occupation).  watch(x) / watchWith(x, m) by actor a: x == a is a no-op; a slot that
 * holds x and is watching or due makes the same kind with the same message a no-op and anything else an
 * IllegalStateException (checkWatchingSame): the rest of the case's actions is skipped, the message counts as
 * delivered, the actor stops, `conflicts` grows; a notified slot holding x makes it a no-op; otherwise the lowest
 * free slot becomes watching; with no free slot AGX_ECAPACITY is raised (sticky) and the watch is not recorded
 * (the one bounded difference: the reference's `watching` map is unbounded).  unwatch(x) frees the slot in any
 * state; a Terminated already enqueued is discarded at receipt, by generation.  A stop frees all the actor's
 * slots; a become leaves them alone.
 * At the end of every tick e each watching slot whose watchee's death tick is <= e - 1 becomes due (a death in
 * e itself is never seen at the end of e); at the entry of tick e + 1 each due slot becomes notified and a
 * Terminated envelope enters the watcher's own inbox, after the backlog, the arrivals and the host-staged
 * tells, in slot order: sender = the watchee, payload = AGX_TAG_WATCH << 24 | slot << 22 | (generation mod
 * 2^22).  It is admitted by position like any message (a dead letter in a full bounded mailbox; its slot then
 * stays notified until unwatch or stop).  So a death at tick s reaches its watchers' inboxes at s + 2, and a
 * watch at tick s of an actor that died before s is answered at s + 1.
 * Receipt: a drained message with tag AGX_TAG_WATCH takes a drain slot and counts as delivered; if the slot is
 * not notified or its generation differs it is discarded (`discarded`, not unhandled); otherwise the slot
 * becomes free and, with a custom message, the ordinary cases run on it with AGX_V_SENDER = the watchee, else
 * the signal cases (AGX_CASE_SIGNAL) run; if none matches that is the death pact: the actor stops,
 * `death_pacts` grows (DeathPactException, ActorAdapter.scala:200-205).
 * Conservation: staged + emitted + terminated = delivered + dead_letters + in_flight.  The engine is active at
 * the entry of tick t iff mail is in flight, or a slot is due, or some actor stopped in tick t - 1 while at
 * least one slot of the engine was watching at the end of t - 1; a run ends at the first tick at whose entry the
 * engine is not active, and agx_run(n) lets exactly min(n, ticks until then) ticks pass.
 * Tag AGX_TAG_WATCH is reserved: agx_stage_tells / agx_tell refuse it (AGX_EINVAL).
 * Call before the first agx_run (AGX_ESTATE afterwards).  AGX_EINVAL: n_slots outside 1..4, n_ranks > 1, an
 * engine with a CRDT kind, a priority table, a stash class or timers (either call order), an engine whose
 * bounded-mailbox ring pool exists, max_emit > 1.  AGX_ENOMEM: the slots do not fit.  Such an engine uses no
 * wave, ring, dense or persistent launch, and a bucket whose inbox -- backlog and the tick's Terminated
 * envelopes included -- exceeds one 2048-message tile makes agx_run return AGX_ECAPACITY (sticky).  Tables with
 * a watch action or a signal case on an engine without death watch make agx_run return AGX_EINVAL. */
agx_status agx_set_death_watch(agx_engine* eng, uint32_t n_slots);
/* The setup block (before the first run or between runs): actor first_id + i watches watchees[i], or
 * (first_id + i + offset) mod n_actors when watchees is NULL; with_message != 0: watchWith(.., payload).
 * Stopped actors are skipped; the rules are those of a device watch, conflicts included (a conflicting actor is
 * stopped and counted).  A host start happens between ticks: a watchee that is dead by then makes the slot due
 * at once, and its Terminated arrives in the next tick.  AGX_EINVAL on an engine without death watch (and the
 * engine's agx_run then returns AGX_EINVAL too). */
agx_status agx_start_watch(agx_engine* eng, uint64_t first_id, uint64_t count, const uint32_t* watchees, int64_t offset,
                           int32_t with_message, uint32_t payload);
/* Totals since agx_create: slots occupied by a watch, Terminated envelopes sent (those that died at admission
 * included), envelopes discarded at receipt, death pacts, conflicts; right now: watching slots, pending (due)
 * slots; and ticks: the supersteps that ran while the engine was active.  Any pointer may be NULL. */
agx_status agx_watch_info(agx_engine* eng, uint64_t* watches, uint64_t* terminated, uint64_t* discarded,
                          uint64_t* death_pacts, uint64_t* conflicts, uint64_t* watching, uint64_t* pending,
                          uint64_t* ticks);
/* One actor's watch slots (for tests and tools): state 0 free, 1 watching, 2 due, 3 notified, | 4 with a custom
 * message.  Slots past n_slots read as zero.  Any pointer may be NULL. */
agx_status agx_read_watch(agx_engine* eng, uint64_t actor_id, uint32_t watchee[4], uint32_t state[4], uint32_t payload[4],
                          uint32_t generation[4]);

/* Supervision (Behaviors.supervise(..).onFailure(strategy), the PreRestart and PostStop signals:
 * TY/internal/Supervision.scala:43-52,128-160,311-406, pinned by SupervisionSpec.scala:100-245; DESIGN.md 2.5 has
 * the contract).
 * A compiled case may end in AGX_RES_FAIL: its actions run, the message counts as delivered, `failures` grows
 * and agx_case.next is the exception class.  agx_set_supervision gives compiled behaviour b the entries
 * table[b * n_levels .. + n_levels), inner first; an entry with class_mask 0 catches nothing.  The entries
 * that count for an actor are those of the kind it was registered with; they stay in force across become.
 * A failure goes to the first entry whose mask has the class.  No such entry, or AGX_SUP_STOP: the actor
 * stops.  AGX_SUP_RESUME: behaviour and state stay as the case left them.  AGX_SUP_RESTART at tick t with the
 * entry's count c and deadline d (none at first; time is left iff there is none or t <= d): if max_restarts
 * != -1, c >= max_restarts and time is left, the failure passes to the next outer entry whose mask matches
 * (none: the actor stops).  Otherwise the PreRestart signal runs on the current behaviour, c becomes c + 1
 * (1 if no time was left), d stays if it exists and time is left and else becomes t + within, every inner
 * entry's count and deadline are cleared, the kind becomes the initial kind, the state words of reset_mask take
 * their reset values, and the drain goes on with the next message under the restarted behaviour.
 * AGX_SIGNAL_PRERESTART / AGX_SIGNAL_POSTSTOP run the matching supervision signal cases of the behaviour current at
 * that moment, inside the drain (no envelope, no tag reserved); PostStop runs at every stop of an actor (a
 * `stopped` result, a failure that stops).  A supervision signal case's actions apply, its result must be
 * AGX_RES_SAME (AGX_EINVAL at agx_set_behaviors otherwise); no matching case is not unhandled.  Its tells
 * count as emitted.  Within one behaviour the tells of a case that fails or stops plus the tells of the
 * largest supervision signal case may not exceed max_emit (1): agx_run refuses such tables (AGX_EINVAL).
 * A tick is a superstep with mail: ticks == agx_stats.supersteps; time does not pass between runs.
 * Call before the first agx_run (AGX_ESTATE afterwards).  AGX_EINVAL: n_levels outside 1..4, n_behaviors
 * outside 1..64, a bad entry, n_ranks > 1, an engine with a CRDT kind, a priority table, a stash class, timers
 * or death watch (either call order), an engine whose bounded-mailbox ring pool exists, max_emit > 1.  Such an
 * engine uses no wave, ring, dense or persistent launch, and a bucket whose inbox exceeds one 2048-message
 * tile makes agx_run return AGX_ECAPACITY (sticky).  Tables with AGX_RES_FAIL or a supervision signal case on
 * an engine without supervision, and tables with watch, timer or stash content on an engine with it, make
 * agx_run return AGX_EINVAL.  restartWithBackoff comes on top (agx_set_backoff below).  Left out: children,
 * supervise around a behaviour reached by become, logging. */
#define AGX_MAX_SUPERVISORS 4u
#define AGX_SUP_RESUME 1u
#define AGX_SUP_RESTART 2u
#define AGX_SUP_STOP 3u
typedef struct agx_supervisor {
  uint32_t class_mask;  /* bit c: the entry catches exception class c; 0: the entry is unused            */
  uint8_t strategy;     /* AGX_SUP_RESUME / _RESTART / _STOP                                              */
  uint8_t reset_mask;   /* RESTART: bit w = state word w (0, 1) takes reset[w]; the others stay           */
  uint8_t pad[2];
  int32_t max_restarts; /* RESTART: -1 = unlimited                                                        */
  uint32_t within;      /* RESTART: the window of max_restarts in ticks, >= 1                             */
  uint64_t reset[2];
} agx_supervisor; /* 32 bytes */
agx_status agx_set_supervision(agx_engine* eng, const agx_supervisor* table, uint32_t n_behaviors, uint32_t n_levels);
/* Totals since agx_create: failures (AGX_RES_FAIL results), resumes, restarts, stops (every stop of an actor
 * inside a drain), and ticks: the supersteps with mail so far.  Any pointer may be NULL. */
agx_status agx_supervision_info(agx_engine* eng, uint64_t* failures, uint64_t* resumes, uint64_t* restarts,
                                uint64_t* stops, uint64_t* ticks);
/* One actor (for tests and tools): the kind it was registered with, and per level the restart count and the
 * ticks left of its window (deadline - ticks so far, 0 once it has passed; 0xFFFFFFFF when there is no
 * deadline).  Levels past n_levels read as 0 / 0xFFFFFFFF.  Any pointer may be NULL. */
agx_status agx_read_supervision(agx_engine* eng, uint64_t actor_id, uint32_t* initial_kind, uint32_t count[4],
                                uint32_t remaining[4]);

/* restartWithBackoff (SupervisorStrategy.restartWithBackoff(min, max, randomFactor) with withMaxRestarts,
 * withResetBackoffAfter and withStashCapacity: TY/internal/Supervision.scala:163-406, pinned by SupervisionSpec.scala:
 * 370-422,774-924; DESIGN.md 2.14 has the contract).  Backoff sits on top of supervision: agx_set_backoff comes after
 * agx_set_supervision, with the same n_behaviors and n_levels, before the first run, once.  Row table[b * n_levels +
 * k] turns the AGX_SUP_RESTART entry of the same place into a backoff entry; a row with min_backoff == 0 leaves the
 * entry a plain restart.  The entry's max_restarts is withMaxRestarts, its `within` is ignored.
 * A failure caught by a backoff entry at tick t, the entry having the count c and a reset-due r (none at first):
 * r exists and t >= r: c = 0, r = none.  Then, if max_restarts != -1 and c >= max_restarts, the actor stops
 * (PostStop); unlike a plain restart the failure does not pass to an outer entry.  Otherwise PreRestart runs, c
 * becomes c + 1, the inner entries are cleared, kind and reset words are re-created as by a restart, and the actor is
 * suspended: delay = c >= 30 ? max_backoff : min(max_backoff, min_backoff << c), plus (delay * random_factor_q16 *
 * r16) >> 32 with r16 the top 16 bits of the counter RNG (the seed of agx_set_fanout / agx_set_gossip, 0 without;
 * the actor's id; t); until = t + delay, r = until + reset_after (both saturate at 2^32 - 1).
 * The failing message counts as delivered and the drain window ends there.  While t < until nothing addressed to
 * the actor is processed: the queue behind the failing message is cut to its first stash_capacity items and stays
 * queued, in order; in later ticks an arrival is admitted while the held length is below min(mailbox capacity,
 * stash_capacity).  What is cut or refused is a dead letter and counts as `dropped`.  stash_capacity -1 is the
 * mailbox capacity (none of its own on an unbounded mailbox; the reference's configured default is 1000).  Held
 * mail is in flight: a run to quiescence lets the delay pass.  From tick `until` on the actor drains as always.
 * AGX_EINVAL, each with its own message: before agx_set_supervision, a second call, other dimensions than
 * agx_set_supervision's, a bad row (1 <= min_backoff <= max_backoff <= 2^31 - 1, random_factor_q16 <= 65536,
 * reset_after >= 1, stash_capacity >= -1), a row on a level whose entry is not AGX_SUP_RESTART.  AGX_ESTATE after
 * the first run.  agx_set_supervision with another table drops the rows.  Every refusal of the supervision engine is
 * inherited.  Left out: stopChildren, stashing of signals, withLoggingEnabled. */
typedef struct agx_backoff {
  uint32_t min_backoff, max_backoff; /* ticks; min_backoff 0: the entry stays a plain restart                     */
  uint32_t random_factor_q16;        /* 0..65536: the jitter's factor in 1/65536                                  */
  uint32_t reset_after;              /* ticks after `until` at which the count resets, >= 1                       */
  int32_t stash_capacity;            /* >= -1; -1: the mailbox capacity                                           */
} agx_backoff; /* 20 bytes */
agx_status agx_set_backoff(agx_engine* eng, const agx_backoff* table, uint32_t n_behaviors, uint32_t n_levels);
/* Totals since agx_create: backoffs (suspensions), resumed (suspensions that have ended: backoffs - suspended),
 * dropped (messages cut or refused by a stash bound), limit_stops (stops by withMaxRestarts), and the actors
 * suspended now (those that will not drain in the next tick).  Any pointer may be NULL. */
agx_status agx_backoff_info(agx_engine* eng, uint64_t* backoffs, uint64_t* resumed, uint64_t* dropped,
                            uint64_t* limit_stops, uint64_t* suspended);
/* One actor: the coming ticks during which it stays suspended (0: it drains in the next tick) and the tick at which
 * it drains again (0: never suspended).  For a backoff level agx_read_supervision's `remaining` is the ticks until
 * the count resets.  Any pointer may be NULL. */
agx_status agx_read_backoff(agx_engine* eng, uint64_t actor_id, uint32_t* suspended_for, uint32_t* until);

/* Child actors (context.spawn / context.stop(child) and the parent's stop taking its children: AA/dungeon/
 * Children.scala, TY/internal/adapter/ActorContextAdapter.scala:79-106, pinned by ActorContextSpec.scala:214-240,
 * 336-428,656-, GracefulStopSpec.scala:20-48, RoutersSpec.scala:40-104; DESIGN.md 2.6 has the contract).
 * Children live on an engine with death watch: agx_set_children is AGX_EINVAL before agx_set_death_watch, and
 * the slot count cannot change afterwards.  They inherit that engine's refusals (n_ranks > 1, max_emit > 1,
 * timers, a stash, priority tables, supervision, CRDT kinds, the one-tile limit of a bucket's inbox).
 * Ids are laid out by regions: the k-th spawn (k = 0, 1, ...) of parent p of a region creates id first_child +
 * (p - first_parent) * max_children + k; ids are never reused and the parent of an id is computed from this
 * formula.  Parent ranges are pairwise disjoint; child blocks (n_parents * max_children ids from first_child) are
 * pairwise disjoint and lie in [0, n_actors); a region's child block may lie inside another region's parent range
 * (grandchildren) but not overlap its own; child-block ids must be unregistered when the first run starts, and
 * agx_register_range into a child block is refused (either call order).  Their death tick starts as "none" (not
 * "dead before tick 1"): a watch on an id that is never created never fires (the one bounded difference).
 * A spawn site says what a child starts as: its kind (a compiled behaviour), state word 0 = base0 + the spawn's
 * argument (low AGX_SPAWN_ARG_BITS bits), state word 1 = word1 or, with AGX_SITE_WORD1_PARENT, the parent's id.
 * AGX_A_SPAWN by actor p at tick s: p in no parent range or p's block full -> refused (`refused`, the receiving
 * word reads 0xFFFFFFFF, nothing is sent, the run goes on); else the spawn count and `spawned` grow, the word takes
 * the child id and a Create envelope (sender p, payload AGX_TAG_CREATE << 24 | site << 18 | argument) goes to the
 * child through the case's tell slot and counts as emitted.  AGX_A_STOP_CHILD(ref): ref one of the actor's spawned
 * children -> a Stop envelope (AGX_TAG_STOP << 24) the same way; any other value, the actor itself included, is
 * the IllegalArgumentException: the rest of the case's actions is skipped, the message counts as delivered, the
 * actor stops, `illegal_stops` grows.
 * Receipt: Create and Stop envelopes are system messages.  One arriving in tick t is consumed at the start of
 * the tick, wherever it stands in the inbox; it takes no mailbox capacity and no drain slot, is never queued, a
 * dead letter or unhandled, and counts as delivered.  All Creates of an actor are looked at before its Stops, each
 * in inbox order.  A Create from the id's computed parent, for an id never created, with a valid site, is
 * effective: the actor is alive from this tick on with the site's kind and state (`created`), and the tick's other
 * mail is admitted as for any live actor.  A Stop from the computed parent to a live created child is effective:
 * the child stops at the start of the tick as by Behaviors.stopped (death tick t, watch slots freed,
 * `child_stops`), and all its mail of the tick is dead letters.  Every other Create or Stop: `discarded`.
 * At the end of tick e every live created child whose computed parent has a death tick <= e - 1 stops (death tick
 * e, slots freed, `cascade_stops`): a subtree dies one level per tick, and a parent's watchers may hear of its
 * death before its deep descendants are gone (the reference's parent terminates after its children: the second
 * bounded difference).  The scan runs only in a tick after one in which an actor stopped in the engine.
 * The engine is active at the entry of tick t also if an actor stopped in t - 1 while a created child was alive at
 * the end of t - 1.  Conservation keeps its form.  Tags 0xFD and 0xFC are reserved like 0xFE.
 * Call before the first agx_run (AGX_ESTATE afterwards).  AGX_EINVAL: no death watch, more than
 * AGX_MAX_CHILD_REGIONS regions or AGX_MAX_SPAWN_SITES sites, a layout rule broken, a registered id in a child
 * block, a site whose kind is no compiled behaviour kind. */
typedef struct agx_child_region {
  uint32_t first_parent, n_parents, first_child, max_children;
} agx_child_region;
#define AGX_SITE_WORD1_PARENT 1u
typedef struct agx_spawn_site {
  uint32_t kind, flags;
  uint64_t base0, word1;
} agx_spawn_site;
agx_status agx_set_children(agx_engine* eng, const agx_child_region* regions, uint32_t n_regions,
                            const agx_spawn_site* sites, uint32_t n_sites);
/* The setup block (Behaviors.setup { ctx => ctx.spawn(..) }), before the first run or between runs: every live
 * actor of [first_parent, first_parent + count) spawns once by the rules of AGX_A_SPAWN; its Create arrives in the
 * next tick.  Such a Create travels with the host-staged tells and counts as staged, not emitted. */
agx_status agx_spawn_children(agx_engine* eng, uint64_t first_parent, uint64_t count, uint32_t site, uint32_t arg);
/* Totals since agx_create (see above) and the created children alive right now.  Any pointer may be NULL. */
agx_status agx_children_info(agx_engine* eng, uint64_t* spawned, uint64_t* refused, uint64_t* created,
                             uint64_t* child_stops, uint64_t* cascade_stops, uint64_t* illegal_stops,
                             uint64_t* discarded, uint64_t* live);
/* One actor: its computed parent (0xFFFFFFFF: none), its spawn count, whether it was ever created. */
agx_status agx_read_children(agx_engine* eng, uint64_t actor_id, uint32_t* parent, uint32_t* spawn_count,
                             uint32_t* created);

/* The receptionist and group routers (Receptionist / ServiceKey / Routers.group: TY/internal/receptionist/
 * LocalReceptionist.scala:147-248, TY/internal/routing/GroupRouterImpl.scala:114-146, RoutingLogic.scala:42-75;
 * pinned by LocalReceptionistSpec.scala:48-133,207-250, RoutersSpec.scala:120-207, RoutingLogicSpec.scala:20-123;
 * DESIGN.md 2.8 has the contract).  A top-level feature: a single-rank engine with max_emit 1, no CRDT kinds, no
 * other feature, no ring pool; call before the first agx_run (AGX_ESTATE afterwards); a second call is AGX_EINVAL.
 * n_keys service keys (1..AGX_MAX_SERVICE_KEYS), every actor holds one bit per key.  AGX_A_REGISTER / DEREGISTER
 * set / clear the actor's own bit; a stop of any cause clears all of them.  The listing of key k in force during
 * tick t is the ids whose bit k was set at the end of tick t - 1, ascending; it holds at most `capacity` ids (a
 * listing that would exceed it is cut to its first `capacity` ids and raises a sticky AGX_ECAPACITY).  version[k]
 * grows by one at the end of every tick in which some actor's bit k differs from its value at the start of the
 * tick.  A bucket's inbox is limited to one tile of 2048 messages (sticky AGX_ECAPACITY). */
agx_status agx_set_receptionist(agx_engine* eng, uint32_t n_keys, uint32_t capacity);
/* The setup block (Behaviors.setup { ctx => receptionist ! Register(key, ctx.self) }), before the first run or
 * between runs: set (on != 0) or clear bit `key` of the live actors of [first_id, first_id + count); the listing
 * is rebuilt at once, in force for the next tick. */
agx_status agx_register_services(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t key, uint32_t on);
/* The listing of `key` in force for the next tick: up to `cap` ids into out_ids, its size into out_n. */
agx_status agx_read_listing(agx_engine* eng, uint32_t key, uint32_t* out_ids, uint64_t cap, uint64_t* out_n);
/* The key masks (bit k = registered under key k) of actors [first, first + count). */
agx_status agx_read_services(agx_engine* eng, uint64_t first, uint64_t count, uint8_t* out_masks);
/* Totals since agx_create: routed (a ROUTE that found a routee), no_routees (one that found none: the reference's
 * Dropped), registered (0 -> 1 changes of a bit), deregistered (1 -> 0 by an action or agx_register_services),
 * terminated (1 -> 0 by a stop), rebuilds (listings rebuilt), and per key the size of the listing in force for the
 * next tick and its version.  Any pointer may be NULL. */
agx_status agx_receptionist_info(agx_engine* eng, uint64_t* routed, uint64_t* no_routees, uint64_t* registered,
                                 uint64_t* deregistered, uint64_t* terminated, uint64_t* rebuilds, uint32_t size[8],
                                 uint64_t version[8]);

/* Pub-sub topics (akka.actor.typed.pubsub.Topic: TY/internal/pubsub/TopicImpl.scala:60-143; pinned by
 * LocalPubSubSpec.scala:20-50,95-156; DESIGN.md 2.10 has the contract), on top of the receptionist: call after
 * agx_set_receptionist and before the first agx_run (AGX_ESTATE afterwards); a second call and a call without the
 * receptionist are AGX_EINVAL.  The engine's service keys are topics as well: subscribing is registering
 * (AGX_A_REGISTER / AGX_A_DEREGISTER, agx_register_services; a stop unsubscribes), AGX_V_LISTING_SIZE is the
 * subscriber count.  The publications of tick s (AGX_A_PUBLISH, agx_publish) are delivered in tick s + 1, each to
 * every actor whose bit `key` is set when the inbox of tick s + 1 is formed (the publisher included, if subscribed),
 * as the last items of the inbox: device publications in (publisher id, index within its drained window) order,
 * then host publications in call order.  Admission is unchanged; the sender of a delivery is the publisher.
 * A tick holds at most log_capacity publications (1..65536; one more raises a sticky AGX_ECAPACITY); a bucket's
 * inbox, deliveries included, is limited to one tile of 2048 messages as on every engine with the receptionist.
 * Conservation: staged + emitted + fanned_out = delivered + dead_letters + in_flight; planned deliveries are in
 * flight, and an engine with any pending is not quiescent. */
#define AGX_MAX_TOPIC_LOG 65536u
agx_status agx_set_topics(agx_engine* eng, uint32_t log_capacity);
/* topic ! Publish(msg) from the host, before the first run or between runs: appended to the log the next tick
 * delivers, after any publication the device left there.  `sender` may be AGX_NO_SENDER.  AGX_EINVAL on an engine
 * without topics or for a key the receptionist does not have. */
agx_status agx_publish(agx_engine* eng, uint32_t key, uint32_t sender, uint32_t payload);
/* Totals since agx_create: published (AGX_A_PUBLISH actions run), fanned_out (delivery envelopes created),
 * no_subscribers (publications that found no recipient: the reference's Dropped; neither dead letters nor emitted),
 * host_published (agx_publish calls applied).  A re-plan after agx_register_services between a publication and its
 * delivery corrects fanned_out and no_subscribers.  Any pointer may be NULL; zeros on an engine without topics. */
agx_status agx_topic_info(agx_engine* eng, uint64_t* published, uint64_t* fanned_out, uint64_t* no_subscribers,
                          uint64_t* host_published);
/* The pending log (the publications the next tick delivers), in delivery order: up to `cap` entries into out_key /
 * out_sender / out_payload (each may be NULL), their number into out_n. */
agx_status agx_read_topic_log(agx_engine* eng, uint32_t* out_key, uint32_t* out_sender, uint32_t* out_payload,
                              uint64_t cap, uint64_t* out_n);

/* Receptionist.Subscribe / Find and the Listing message (TY/internal/receptionist/LocalReceptionist.scala:152-171,
 * 209-220,233-238; pinned by LocalReceptionistSpec.scala:81-175; DESIGN.md 2.11 has the contract), on top of topics:
 * call after agx_set_topics and before the first agx_run (AGX_ESTATE afterwards); a second call, a call without
 * topics and an n_keys other than the receptionist's are AGX_EINVAL.  listing_payload[k] is the payload of a Listing
 * envelope of key k (its message tag in bits 24..31); its sender is AGX_NO_SENDER.  Every actor holds two more masks:
 * `sub` (bit k: subscribed to key k) and `pending` (bit k: one Listing of key k is owed at the next tick).
 * AGX_A_SUBSCRIBE_LISTING sets both of the actor's own bits (also when repeated), AGX_A_FIND the pending bit only; a
 * stop of any cause clears both masks; there is no unsubscribe on the device.  Key k changed in tick s when
 * version[k] moved at the end of tick s, or when agx_register_services changed a bit between two runs.  When the inbox
 * of tick s + 1 is formed, an alive actor receives exactly one Listing(k) if its pending bit k is set, or if k changed
 * and its sub bit k is set; the pending bits served are cleared.  The Listings are the last items of the inbox, after
 * the publications, in ascending key and, per key, ascending id; admission is by position.  The handler reads the set
 * through AGX_V_LISTING_SIZE / AGX_V_SERVICE_AT: the listing in force in the tick the message is drained (a Listing
 * queued by a throughput cap sees a newer one).  Owed Listings are in flight: staged + emitted + fanned_out +
 * listings_sent = delivered + dead_letters + in_flight.  A bucket's inbox, Listings included, is limited to one tile
 * of 2048 messages as on every engine with the receptionist.  Tables with the two actions on an engine without
 * listings, or with a key the receptionist does not have, make agx_run return AGX_EINVAL. */
agx_status agx_set_listings(agx_engine* eng, const uint32_t* listing_payload, uint32_t n_keys);
/* The setup block (Behaviors.setup { ctx => receptionist ! Subscribe(key, ctx.self) }), before the first run or
 * between runs, for the live actors of [first_id, first_id + count): on != 0 sets `sub` and `pending` (the initial
 * Listing arrives in the next tick); on == 0 clears `sub` (a convenience of the host; a pending bit stays).
 * AGX_EINVAL on an engine without listings or for a key the receptionist does not have. */
agx_status agx_subscribe_listings(agx_engine* eng, uint64_t first_id, uint64_t count, uint32_t key, uint32_t on);
/* Totals since agx_create: subscribes / finds (actions run, plus the members of an agx_subscribe_listings range with
 * on != 0 whose masks changed), listings_sent (Listing envelopes created), notified (key-ticks in which a changed key
 * had at least one recipient).  A re-plan after a host call between a change and its Listings corrects listings_sent
 * and notified.  Any pointer may be NULL.  AGX_EINVAL on an engine without listings. */
agx_status agx_listing_info(agx_engine* eng, uint64_t* subscribes, uint64_t* finds, uint64_t* listings_sent,
                            uint64_t* notified);
/* The `sub` and `pending` masks of actors [first, first + count) (either pointer may be NULL). */
agx_status agx_read_subscriptions(agx_engine* eng, uint64_t first, uint64_t count, uint8_t* sub_out, uint8_t* pending_out);

/* Consistent-hashing and random routing for group routers (Routers.group(key).withConsistentHashingRouting /
 * withRandomRouting: TY/internal/routing/RoutingLogic.scala:77-112, akka-actor routing/ConsistentHash.scala:25-139,
 * routing/MurmurHash.scala:115-129; pinned by RoutingLogicSpec.scala:146-221; DESIGN.md 2.12 has the contract), on
 * top of the receptionist: call after agx_set_receptionist and before the first agx_run (AGX_ESTATE afterwards).
 * AGX_EINVAL: no receptionist, topics set (agx_set_topics after this call is refused too), a bit of
 * hashed_keys_mask at or above the receptionist's n_keys, a non-zero mask with virtual_nodes_factor outside
 * 1..AGX_MAX_VIRTUAL_NODES or with n_actors x virtual_nodes_factor above AGX_MAX_RING_POINTS, a second call.  With
 * hashed_keys_mask 0 (random routing only) virtual_nodes_factor is ignored.  A node is an actor id as an unsigned
 * decimal string; ring point v (1..virtual_nodes_factor) of actor a is concatenateNodeHash(stringHash(str(a)), v).
 * The ring of a hashed key k in force during tick t is the ring points of the actors whose bit k was set at the end
 * of tick t - 1, ordered by (hash as a signed 32-bit integer, id).  AGX_A_ROUTE with AGX_ROUTE_HASHED sends to the
 * id of the first ring entry with hash >= stringHash(str(x)) (signed), else to that of entry 0; an empty ring is an
 * empty listing (a dead letter, no_routees).  AGX_ROUTE_RANDOM sends to listing[fanout_rand(seed, self,
 * (c & 0xFFFFFF) | 0x02000000, 0) mod size], c the low 32 bits of state word `word`, which grows by one on a hit.
 * Tables that use either flag on an engine without this call, AGX_ROUTE_HASHED on a key outside the mask, or two of
 * BY_INDEX / HASHED / RANDOM on one action make agx_run return AGX_EINVAL. */
agx_status agx_set_router_logics(agx_engine* eng, uint32_t hashed_keys_mask, uint32_t virtual_nodes_factor, uint64_t seed);
/* Totals since agx_create: hashed / random (routes of that logic that found a routee; they are part of `routed`),
 * ring_rebuilds (rings rewritten after a change of their key), and per key the size of the ring in force for the
 * next tick in ring points.  Any pointer may be NULL; zeros on an engine without router logics. */
agx_status agx_router_info(agx_engine* eng, uint64_t* hashed, uint64_t* random, uint64_t* ring_rebuilds, uint32_t ring_size[8]);
/* The ring of hashed key `key` in force for the next tick, in ring order: up to `cap` hashes / ids into out_hash /
 * out_id (either may be NULL), its size into out_n.  AGX_EINVAL without router logics or for a key outside the mask. */
agx_status agx_read_hash_ring(agx_engine* eng, uint32_t key, uint32_t* out_hash, uint32_t* out_id, uint64_t cap,
                              uint64_t* out_n);

/* --- the reply path: actors that live on the host ------------------------------------------
 * Ids [first_host_id, first_host_id + n_host) -- outside the population (>= n_actors, < 2^31) --
 * name host-side actors, e.g. the JVM ActorRefs that told GPU actors (their sender() ids).  A GPU
 * behaviour's tell to one of them is not a dead letter: it is appended to the engine's outbox
 * (each sender's tells in emission order; different senders interleave arbitrarily, as on the
 * JVM) and the host takes it with agx_take_outbound and delivers it.  Outbound tells leave the
 * engine: they are not counted in agx_stats.emitted.  More than `capacity` outbound tells between
 * two agx_take_outbound calls is AGX_ECAPACITY.  agx_take_outbound copies up to `cap` envelopes
 * (dst host id, src GPU actor id, payload) and removes them; *n = how many.                   */
agx_status agx_set_outbound(agx_engine* eng, uint32_t first_host_id, uint32_t n_host, uint64_t capacity);
agx_status agx_take_outbound(agx_engine* eng, uint32_t* dst, uint32_t* src, uint32_t* payload, uint64_t cap,
                             uint64_t* n);

/* --- state readback ----------------------------------------------------------- */
/* The population (agx_cfg.n_actors, all ranks) and state words per actor: the sizes a binding
 * checks caller arrays against before agx_set_graph / agx_read_state (whose pointers carry none). */
agx_status agx_get_shape(agx_engine* eng, uint64_t* n_actors, uint32_t* n_words);
/* words: count x n_words u64 (actor-major); alive: count bytes (may be NULL).
 * Only ids owned by this rank are written; others are left untouched.       */
agx_status agx_read_state(agx_engine* eng, uint64_t first_id, uint64_t count, uint64_t* words,
                          uint8_t* alive);

/* --- multi-GPU (one process per GPU, RCCL over xGMI) ------------------------- */
/* 128-byte RCCL unique id: rank 0 creates it, the host broadcasts it.        */
agx_status agx_comm_unique_id(uint8_t out[128]);
agx_status agx_comm_init(agx_engine* eng, const uint8_t id[128]);
/* Single-process loopback transport: run `n` engines (ranks 0..n-1 of one
 * population) that share one device, exchanging mail with device copies.
 * Same kernels as the RCCL path; used to test sharding on a 1-GPU box.      */
agx_status agx_group_run(agx_engine** engs, uint32_t n, uint32_t max_supersteps, agx_stats* out);

/* The device-resident replays' per-superstep decision (pure host function, no GPU; the device runs
 * the same code in k_mr_pack / k_mr_unpack, agx_kernels.h mr_decide).  `mat` as below; `slab` =
 * envelopes per fixed-size peer slab; `cap` = this rank's message capacity.  *code: 0 = exchange
 * the slabs, 1 = some sender -> receiver count (off the diagonal) exceeds the slab (the host redoes
 * this superstep's exchange exactly and grows the slabs), 2 = nothing in flight on any rank, 3 =
 * backlog + received mail would exceed `cap`.  send_off / recv_off: R + 1 entries (exclusive
 * prefixes of this rank's send counts and of its receive counts in sender-rank order; [R] = the
 * total); *n_backlog = this rank's backlog (received mail is placed after it).
 * Replaces: ShardRegion delivery to remote regions (akka-cluster-sharding/.../ShardRegion.scala:
 * 154-158 routing), batched once per superstep. */
agx_status agx_mr_plan(const uint64_t* mat, uint32_t n_ranks, uint32_t rank, uint32_t slab, uint64_t cap,
                       uint32_t* code, uint64_t* send_off, uint64_t* recv_off, uint64_t* n_backlog);

/* Exchange plan of one superstep (pure host function, no GPU).  `mat` is the
 * gathered R x (R+2) matrix, row r = rank r's [tells to rank 0..R-1,
 * n_backlog, n_staged].  Outputs (R entries each): this rank's send
 * counts/offsets into its owner-partitioned tell buffer and receive
 * counts/offsets into its sort input, where received mail follows the local
 * backlog in sender-rank order (the sharded canonical order).  *inflight =
 * global messages in flight (0 = quiescent on every rank).                  */
agx_status agx_exchange_plan(const uint64_t* mat, uint32_t n_ranks, uint32_t rank, uint64_t* send_cnt,
                             uint64_t* send_off, uint64_t* recv_cnt, uint64_t* recv_off, uint64_t* inflight);

/* --- measurement ----------------------------------------------------------- */
/* Per-kernel HIP-event timing on the engine's stream (off by default).      */
agx_status agx_profile_enable(agx_engine* eng, int on);
/* Fills up to `cap` entries; returns the number of kernel classes in *n.
 * items[k]: for "bucket_apply_dense", the profiled dense launches that took
 * every bucket (read from the device's dense_left flags after each launch:
 * the wave / block launches of those supersteps returned at entry); 0 else. */
agx_status agx_profile_read(agx_engine* eng, char (*names)[32], double* total_ms,
                            uint64_t* launches, uint64_t* items, uint32_t cap, uint32_t* n);
agx_status agx_profile_reset(agx_engine* eng);

/* --- sharding helpers (ShardRegion.HashCodeMessageExtractor) ---------------- */
/* (math.abs(entityId.hashCode) % maxNumberOfShards) with entityId = decimal id
 * (akka-cluster-sharding/.../ShardRegion.scala:154-158).  May be negative.  */
int32_t agx_shard_id(uint32_t id, uint32_t num_shards);
/* rank owning `id` = floor-mod(shard_id, n_ranks).                           */
uint32_t agx_owner(uint32_t id, uint32_t num_shards, uint32_t n_ranks);

#ifdef __cplusplus
}
#endif
#endif /* AKKA_GPU_H */
