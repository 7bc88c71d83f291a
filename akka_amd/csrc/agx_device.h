// agx_device.h — device-side building blocks for the gfx950 dispatch engine:
// wave64 / block scans, the behaviour table (typed Behaviors.receive subset)
// and the counter RNG.  Integer only; no MFMA (the path is HBM/scatter-bound).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/akka_gpu.h"

namespace agx {

constexpr int kWave = 64;               // CDNA wavefront
constexpr uint32_t kLocalMask = 0x0FFFFFFFu;  // key = (owner << 28) | local
constexpr int kOwnerShift = 28;

// ------------------------------------------------------------------ params
struct DevParams {
  uint32_t n_global, n_local, W, T, C, R, rank, kmax;
  uint32_t ring_stride, fan_k;  // ring_stride pre-reduced mod n_global
  uint64_t fan_seed, zipf_n;
  const uint32_t* zipf_cdf;
  const uint2* zipf_ent;      // [2^kZipfBits] direct answers / search ranges (see zipf_dest)
  const uint32_t* zipf_perm;
  const uint64_t* row_ptr;  // local rows
  const uint32_t* col;      // global dst ids
  const uint32_t* route;    // global id -> (owner<<28)|local   (R > 1 only)
  const uint32_t* gid;      // local -> global id              (R > 1 only)
  uint8_t* kind;
  uint8_t* alive;           // read-only inside k_apply; stops are committed after it
  uint32_t* stopq;          // actors that returned Behaviors.stopped this step
  uint32_t* nstop;
  uint64_t* state;          // word-major SoA: state[w * n_local + l]; CRDT engines (pw > 0): actor-major,
                            // state[l * pitch + w] (wide_state)
  uint32_t pitch;           // u64 words per actor row of an actor-major engine (0: word-major)
  // words 0 / 1 of a plain behaviour: state[l * sa + w * sw] -- word-major (sa 1, sw n_local), or
  // actor-major pairs of a two-word engine (sa 2, sw 1: one line holds both words of 8 actors, so
  // a sparse superstep touches one state line per activation instead of two)
  uint32_t sa, sw;
  // priority mailboxes (agx_set_mailbox_priority): bit c = mailbox class c has a priority table (ptab below)
  uint32_t pmask;
  // CRDT state gossips (agx_crdt.h): snapshot rows, row-major, `pw` u32 each.
  // heap = 2 x heap_rows rows (ping-pong by superstep parity); rx = rows
  // received from other ranks this superstep (handle - heap_rows).
  uint32_t* heap;
  // (an engine has CRDT kinds or priority mailboxes, never both -- agx_set_mailbox_priority: one slot)
  union {
    const uint32_t* rx;
    // priority mailboxes, read only by the prioritised k_bucket_apply instantiations: the classes' tables
    // ptab[class * 256 + tag] (lower = dequeued first), then one byte per bucket, != 0 when the bucket
    // holds an actor of a prioritised class (kPrioBucketOff; written on the host when mailboxes are bound)
    const uint8_t* ptab;
    // deque-based mailboxes (agx_set_stash), read and written only by the stash k_bucket_apply instantiations:
    // the per-actor stash buffers and their bookkeeping (StashDev below)
    uint32_t* stash;
    // timers (agx_set_timers), read and written only by the timer k_bucket_apply instantiations: the
    // per-actor timer slots and their bookkeeping (TimerDev below)
    uint32_t* timers;
    // death watch (agx_set_death_watch), read and written only by the watch k_bucket_apply instantiations: the
    // per-actor watch slots, the death ticks and their bookkeeping (WatchDev below)
    uint32_t* watch;
    // supervision (agx_set_supervision), read and written only by the supervision k_bucket_apply instantiations,
    // and only for a message that fails or stops: the strategy entries, the per-actor restart counts and
    // deadlines, the initial kinds and the counters (SuperDev below)
    uint32_t* super;
    // the receptionist (agx_set_receptionist), read and written only by the receptionist k_bucket_apply
    // instantiations and the rebuild kernels: the per-actor key masks, the listings and their bookkeeping
    // (RecepDev below)
    uint32_t* recep;
  };
  uint32_t* heap_top;       // [2] rows allocated in heap[parity]
  const uint32_t* step;     // superstep counter (bumped by the first kernel of a step)
  uint32_t heap_rows, pw, gossip_f;
  uint64_t gossip_seed;
  uint32_t delta_max;             // delta-CRDT mode (Replicator max-delta-size), 0 = off
  unsigned long long* err;        // stats[ST_ERROR]: capacity errors raised inside a behaviour
  // compiled behaviours (agx_set_behaviors): case / action tables, behaviour b = cases [bfirst[b], bfirst[b+1])
  const agx_case* bcase;
  const agx_act* bact;
  const uint32_t* bfirst;
  uint32_t n_beh;
  // the reply path (agx_set_outbound): tells to ids [host_lo, host_lo + host_n) go to the outbox
  uint32_t host_lo, host_n, outbox_cap;
  uint32_t* outbox;     // [outbox_cap][3] dst, src, payload
  uint32_t* outbox_n;   // envelopes appended (may pass outbox_cap: reported as a capacity error)
  // mailbox classes (agx_set_mailbox_class): the class of an actor is bits 1..3 of its alive byte;
  // nmc == 0 -> every actor uses class 0 (C, T above); else capacity mcap[class], drain
  // min(Tr, capacity) (Tr = the dispatcher throughput, >= 1)
  uint32_t nmc, Tr;
  uint32_t mcap[AGX_MAX_MAILBOX_CLASSES];
};

// An actor's bounded capacity (0 = unbounded) and drain limit from its alive byte (bit 0 = alive,
// bits 1..3 = mailbox class): Mailboxes.lookupConfigurator per actor (Mailboxes.scala:204-260).
// actor l's state row in a CRDT engine (actor-major, P.pitch u64 words per row)
__device__ __forceinline__ uint64_t* wide_state(const DevParams& P, uint32_t l) {
  return P.pitch ? P.state + (size_t)l * P.pitch : P.state + l;
}
// the stride between consecutive words of one actor's state (1 actor-major, n_local word-major)
__device__ __forceinline__ size_t wide_nl(const DevParams& P) { return P.pitch ? 1u : P.n_local; }

// word w (0 or 1) of a plain behaviour's state (P.sa / P.sw above; 32-bit offsets)
__device__ __forceinline__ uint32_t sidx(const DevParams& P, uint32_t l, uint32_t w) { return l * P.sa + w * P.sw; }

__device__ __forceinline__ void mbox_limits(const DevParams& P, uint32_t abyte, uint32_t& C, uint32_t& T) {
  if (P.nmc == 0) {  // (uniform: one mailbox type for the whole dispatcher)
    C = P.C;
    T = P.T;
    return;
  }
  C = P.mcap[(abyte >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1)];
  T = C && P.Tr > C ? C : P.Tr;
}

constexpr uint32_t kPrioBucketOff = AGX_MAX_MAILBOX_CLASSES * 256u;  // DevParams.ptab: the per-bucket marks
// Does the actor's mailbox class carry a priority table (P.pmask; class 0 when no classes are set)?
__device__ __forceinline__ bool mbox_prioritised(const DevParams& P, uint32_t abyte) {
  return (P.pmask >> ((abyte >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1))) & 1u;
}
// The priority of a message in that class's queue: the table entry of its tag (payload >> 24);
// lower is dequeued first (PriorityGenerator, Mailbox.scala:726-816; control-aware: 0 / 1, :867-1025)
__device__ __forceinline__ uint32_t mbox_priority(const DevParams& P, uint32_t abyte, uint32_t pay) {
  return P.ptab[((abyte >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1)) * 256u + (pay >> 24)];
}

// ---- deque-based mailboxes: the stash (agx_set_stash; StashBufferImpl.scala:61-79,131-218)
// DevParams.stash, u32 units:
//   [0..7]   stash capacity S of mailbox class c (0: the class has none)
//   [8]      Smax = the largest S: buffer slots per actor   [9] Pmax: park slots per actor
//   [16..21] three u64 counters: stashed, unstashed, overflows
//   [kStashBucketOff + b]       pending: buffered / parked messages bucket b processes next superstep
//                               (counted into the bucket's backlog count, read at the bucket's entry)
//   [kStashBucketOff + nb + b]  != 0: bucket b holds an actor of a class with a stash (host-written)
//   then, 8-byte aligned, one uint2 header per actor (nb << bb of them):
//     x = head | released << 8 | size << 16   (the buffer: a ring of Smax slots starting at head)
//     y = park head | parked << 16            (the park: slots Smax.., consumed from the front)
//   then Smax + Pmax uint2 envelopes (sender, payload) per actor.
constexpr uint32_t kStashBucketOff = 32;
constexpr uint32_t kStashCtr = 16;
struct StashDev {
  uint32_t* base;
  uint2* hdr;
  uint2* slots;
  uint32_t smax, per;  // per = Smax + Pmax envelope slots per actor
  __device__ __forceinline__ uint2* of(uint32_t l) const { return slots + (size_t)l * per; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kStashCtr) + i;
  }
};
__device__ __forceinline__ StashDev stash_dev(const DevParams& P, uint32_t nb, uint32_t bb) {
  StashDev s;
  s.base = P.stash;
  s.smax = P.stash[8];
  s.per = s.smax + P.stash[9];
  const size_t ho = ((size_t)kStashBucketOff + 2u * nb + 1u) & ~(size_t)1;
  s.hdr = reinterpret_cast<uint2*>(P.stash + ho);
  s.slots = s.hdr + ((size_t)nb << bb);
  return s;
}
__device__ __forceinline__ uint32_t stash_cap(const DevParams& P, uint32_t abyte) {
  return P.stash[(abyte >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1)];
}
// the messages a superstep takes from the buffer / the park instead of the mailbox (the source rule):
// the first min(released, T) buffer entries, else the first min(parked, T) parked ones, else none
__device__ __forceinline__ uint32_t stash_window(uint2 h, uint32_t T) {
  const uint32_t rel = (h.x >> 8) & 0xFFu, pc = h.y >> 16;
  return rel ? min(rel, T) : min(pc, T);
}

// ---- timers (agx_set_timers; TY/internal/TimerSchedulerImpl.scala:61-172)
// One superstep is one tick.  DevParams.timers, u32 units:
//   [0]      n_keys: timer slots per actor (1..4)
//   [2]      the last tick at whose entry a bucket had mail or a pending timer (atomicMax; the host's
//            quiescence poll of the multi-pass pipeline and the `ticks` count read it)
//   [4..7]   two u64 counters: fired, discarded
//   [kTmBucketOff + b]           earliest: the tick of bucket b's next fire, kTmNone when no timer is pending
//                                (exact at the end of every tick: a bucket with nothing due reads this word only)
//   [kTmBucketOff + nb + b]      due: the fires of the next tick (counted into the bucket's backlog count, so
//                                the next inbox has room for their TimerMsgs; read at the bucket's entry)
//   [kTmBucketOff + 2 * nb + b]  clock: the ticks bucket b has run (every bucket runs every tick: all equal)
//   then, 16-byte aligned and slot-major ([key][actor], np = nb << bb actors, so a scan of one key over a
//   bucket is coalesced):
//     next[key][np]  the tick of the slot's next fire, kTmNone when none is to come
//     per[key][np]   the period (0: a single timer) | kTmActive
//     gen[key][np]   the slot's generation          pay[key][np]  the message payload
//   then agen[np]: the actor's generation counter minus 1 (the reference's timerGen starts at 1).
// Generations are compared mod 2^22 (the TimerMsg payload carries 22 bits of them).
constexpr uint32_t kTmBucketOff = 16;
constexpr uint32_t kTmLastAct = 2, kTmCtr = 4;
constexpr uint32_t kTmNone = 0xFFFFFFFFu, kTmActive = 0x80000000u, kTmGenMask = 0x3FFFFFu;
constexpr uint32_t kTmMaxDelay = 0x7FFFFFFFu;
__host__ __device__ __forceinline__ size_t tm_slot_off(uint32_t nb) {
  return ((size_t)kTmBucketOff + 3u * (size_t)nb + 3u) & ~(size_t)3;
}
struct TimerDev {
  uint32_t* base;
  uint32_t *next, *per, *gen, *pay, *agen;  // [key * np + l]
  uint32_t nk, np, nb;
  __device__ __forceinline__ uint32_t& earliest(uint32_t b) const { return base[kTmBucketOff + b]; }
  __device__ __forceinline__ uint32_t& due(uint32_t b) const { return base[kTmBucketOff + nb + b]; }
  __device__ __forceinline__ uint32_t& clock(uint32_t b) const { return base[kTmBucketOff + 2u * nb + b]; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kTmCtr) + i;
  }
  __device__ __forceinline__ size_t at(uint32_t key, uint32_t l) const { return (size_t)key * np + l; }
  // cancel: the slot is inactive and nothing of it is to come; the bucket rescans its slots at the end of the tick
  __device__ __forceinline__ void cancel(uint32_t key, uint32_t l, uint32_t b) const {
    const size_t i = at(key, l);
    if (per[i] & kTmActive) {
      per[i] = 0u;
      next[i] = kTmNone;
      atomicMin(&earliest(b), 0u);
    }
  }
  // start: cancel, the actor's next generation, active with the next fire at now + delay (delay in 1..2^31 - 1)
  __device__ __forceinline__ void start(uint32_t key, uint32_t l, uint32_t b, uint32_t now, uint32_t delay, bool periodic,
                                        uint32_t payload) const {
    const size_t i = at(key, l);
    const uint32_t g = agen[l] + 1u;
    agen[l] = g;
    gen[i] = g;
    pay[i] = payload;
    per[i] = (periodic ? delay : 0u) | kTmActive;
    next[i] = now + delay;
    atomicMin(&earliest(b), now + delay);
  }
};
__device__ __forceinline__ TimerDev timer_dev(const DevParams& P, uint32_t nb, uint32_t bb) {
  TimerDev t;
  t.base = P.timers;
  t.nk = P.timers[0];
  t.nb = nb;
  t.np = nb << bb;
  t.next = P.timers + tm_slot_off(nb);
  t.per = t.next + (size_t)t.nk * t.np;
  t.gen = t.per + (size_t)t.nk * t.np;
  t.pay = t.gen + (size_t)t.nk * t.np;
  t.agen = t.pay + (size_t)t.nk * t.np;
  return t;
}
// a computed delay: below 1 counts as 1, above 2^31 - 1 is clamped (the operand is a wrapped 64-bit sum)
__device__ __forceinline__ uint32_t tm_delay(uint64_t d) {
  return (int64_t)d < 1 ? 1u : d > (uint64_t)kTmMaxDelay ? kTmMaxDelay : (uint32_t)d;
}

// ---- receive timeouts (agx_set_receive_timeout; AA/dungeon/ReceiveTimeout.scala:18-74), on top
// of the timers: the same logical time, clocks, due counts and backlog trick.  The timer storage of such an engine
// is longer: after agen[np] come three [actor]-indexed rows
//     rt_next[np]   the tick of the actor's next receive-timeout fire, kTmNone when none is to come
//     rt_delay[np]  the timeout in ticks, 0: none set        rt_pay[np]  the message the behaviour receives
// and the 8 words of the transparent-tag mask (bit t: messages of tag t are NotInfluenceReceiveTimeout).
// Header words [8..11]: two u64 counters, fired and discarded.  On such an engine the bucket's `earliest` word is
// a lower bound of the idle row's fires, not their exact minimum: an influencing receipt pushes a fire later
// without touching it, and the rescan at the end of the tick the bound names re-establishes the exact value.
constexpr uint32_t kRtCtr = 8;
struct IdleDev {
  uint32_t *next, *delay, *pay;
  const uint32_t* mask;
  unsigned long long* ctrs;
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const { return ctrs + i; }
};
__device__ __forceinline__ IdleDev idle_dev(const TimerDev& TD) {
  IdleDev d;
  d.next = TD.agen + TD.np;
  d.delay = d.next + TD.np;
  d.pay = d.delay + TD.np;
  d.mask = d.pay + TD.np;
  d.ctrs = reinterpret_cast<unsigned long long*>(TD.base + kRtCtr);
  return d;
}
// an actor's timeout across its drained window, in registers: the delay, the message, and what the window's
// cases did (kRtChanged: the case set or cancelled -- receiveTimeoutChanged; kRtWasOff: it turned a set timeout off)
constexpr uint32_t kRtChanged = 1u, kRtWasOff = 2u;
struct RtRegs {
  uint32_t delay, pay, flags;
};
// is a message of this tag NotInfluenceReceiveTimeout?  The mask's words live in registers: a select chain, no load
__device__ __forceinline__ bool rt_transparent(const uint32_t (&m)[8], uint32_t tag) {
  const uint32_t i = tag >> 5;
  uint32_t x = m[0];
  x = i == 1u ? m[1] : x;
  x = i == 2u ? m[2] : x;
  x = i == 3u ? m[3] : x;
  x = i == 4u ? m[4] : x;
  x = i == 5u ? m[5] : x;
  x = i == 6u ? m[6] : x;
  x = i == 7u ? m[7] : x;
  return (x >> (tag & 31u)) & 1u;
}

// ---- sharded entities (agx_set_sharding; akka-cluster-sharding Shard.scala:388-516), on top of the
// receive timeouts.  The storage is an allocation of its own whose address stands in the timer storage's header
// words [12..13] (free on an engine with receive timeouts), u32 units:
//   [0]       n_types (1..AGX_MAX_ENTITY_TYPES)
//   [4..15]   six u64 counters (kSc*)
//   [kShTypeOff + kShTypeWords * t]  type t: first_id, count, kind, flags (kShWord1Id), word-0 base lo / hi,
//                                    word 1 lo / hi, stop payload, idle delay, idle payload
//   [kShRowOff ..]  three [actor]-indexed rows of np = nb << bb words:
//     st[np]    the id's incarnation count | kShPassivating
//     pst[np]   the tick of the entity's last stop while passivating (0: none): a start in the tick after it is a restart
//     held[np]  what the entity's last stop left for the next formation to read, then 0:
//               kShHeld | c  stopped while passivating after c messages of its window: the rest of its admitted
//                            inbox stays queued (shard_requeue, this tick)
//               d            a plain stop left d queued messages behind: the old mailbox's, dead at the next formation
constexpr uint32_t kTmShardPtr = 12;
constexpr uint32_t kShCtr = 4, kShTypeOff = 16, kShTypeWords = 12, kShRowOff = kShTypeOff + kShTypeWords * AGX_MAX_ENTITY_TYPES;
constexpr uint32_t kShPassivating = 0x80000000u, kShHeld = 0x80000000u, kShWord1Id = AGX_ENTITY_WORD1_ID;
enum : uint32_t { kScStarted, kScRestarted, kScPassivations, kScPassivated, kScIgnored, kScUnknown, kScN };
struct ShardDev {
  uint32_t* base;
  uint32_t *st, *pst, *held;
  uint32_t nt;
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kShCtr) + i;
  }
  __device__ __forceinline__ const uint32_t* type(uint32_t t) const { return base + kShTypeOff + kShTypeWords * t; }
  // the entity type of id l, nt for an id in no range (at most 8 uniform rows: no search structure)
  __device__ __forceinline__ uint32_t type_of(uint32_t l) const {
    uint32_t r = nt;
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t* T = type(t);
      if (l - T[0] < T[1]) r = t;
    }
    return r;
  }
  // does [a0, a0 + na) meet an entity range?
  __device__ __forceinline__ bool meets(uint32_t a0, uint32_t na) const {
    bool m = false;
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t* T = type(t);
      m |= a0 < T[0] + T[1] && T[0] < a0 + na;
    }
    return m;
  }
};
__device__ __forceinline__ ShardDev shard_dev(const TimerDev& TD) {
  ShardDev s;
  s.base = reinterpret_cast<uint32_t*>(*reinterpret_cast<const unsigned long long*>(TD.base + kTmShardPtr));
  s.nt = s.base[0];
  s.st = s.base + kShRowOff;
  s.pst = s.st + TD.np;
  s.held = s.pst + TD.np;
  return s;
}
// what the drain of one message hands back beside RtRegs: the case ran AGX_A_PASSIVATE
constexpr uint32_t kRtPassivate = 4u;

// ---- ask (agx_set_ask; TY/internal/ActorContextImpl.scala:203-218, TY/scaladsl/AskPattern.scala:
// 109-162), on top of the timers: an outstanding ask is a single timer slot with one more fact about it, the
// timeout is the slot's TimerMsg.  The timer storage of such an engine is longer: after agen[np] comes
//     ask[key][np]  kAskIs (the slot's timer is an ask's timeout) | kAskHasTag | the adapt tag
// read only while the slot is active; every start of a plain timer on the slot clears it.
// Header words [8..15]: four u64 counters, asked, answered, timed out, late.
constexpr uint32_t kAskCtr = 8;
constexpr uint32_t kAskIs = 0x80000000u, kAskHasTag = 0x100u;
enum : uint32_t { kAcAsked, kAcAnswered, kAcTimedOut, kAcLate, kAcN };
struct AskDev {
  uint32_t* row;  // [key * np + l]
  unsigned long long* ctrs;
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const { return ctrs + i; }
};
__device__ __forceinline__ AskDev ask_dev(const TimerDev& TD) {
  AskDev d;
  d.row = TD.agen + TD.np;
  d.ctrs = reinterpret_cast<unsigned long long*>(TD.base + kAskCtr);
  return d;
}
// the ask ref: what the target sees as the sender of a request, and what a reply carries back
__device__ __forceinline__ uint32_t ask_ref(uint32_t key, uint32_t gen, uint32_t id) {
  return AGX_ASK_REF_BIT | (key << AGX_ASK_REF_KEY_SHIFT) | ((gen & AGX_ASK_REF_GEN_MASK) << AGX_ASK_REF_GEN_SHIFT) | id;
}
__device__ __forceinline__ bool is_ask_ref(uint32_t x) { return (x & AGX_ASK_REF_BIT) && x != AGX_NO_SENDER; }
// what a thread's drains counted, in registers: added to the storage once per wave (ask_commit, agx_kernels.h)
struct AskCount {
  uint32_t c[kAcN];
};
// the ask of the case that runs: ARM leaves the ref its SEND puts into the envelope's sender field
struct AskRegs {
  AskDev AD;
  uint32_t ref;
  AskCount* cnt;
};
// The tells of an engine with ask go through this: a tell to an ask ref is the reply -- to the ref's id, with the ref
// in the sender field (the replier's own id is not carried) -- whichever kind emits it; send() is the one envelope of
// an ask, with the ref instead of the asker's id.  The emitter's `self` is swapped for that one call.
template <typename Emit>
struct AskEmit {
  Emit& em;
  __device__ __forceinline__ void send(uint32_t ref, uint32_t dst, uint32_t p) {
    const uint32_t s = em.self;
    em.self = ref;
    em(dst, p);
    em.self = s;
  }
  __device__ __forceinline__ void operator()(uint32_t dst, uint32_t p) {
    if (is_ask_ref(dst)) send(dst, dst & AGX_ASK_REF_ID_MASK, p);
    else em(dst, p);
  }
};

// ---- death watch (agx_set_death_watch; AA/dungeon/DeathWatch.scala:19-113,147-162)
// One superstep is one tick.  DevParams.watch, u32 units:
//   [0]        n_slots: watch slots per actor (1..4)
//   [2]        the last tick at whose entry the engine was active (atomicMax; the host's quiescence poll of the
//              multi-pass pipeline and the `ticks` count read it)
//   [4..13]    five u64 counters: watches, terminated, discarded, death_pacts, conflicts
//   [14..15]   stopw[t & 1]: t once an actor stopped in tick t (writers of tick e write word e & 1, readers at
//              the end of e and at the entry of e + 1 read a word of an earlier launch: no read races a write)
//   [16..17]   anyw[t & 1]: t once a bucket ended tick t with a watching slot
//   [18]       sticky: a watch found no free slot (the end of a tick raises kErrWatchSlots from it)
//   [kWdBucketOff + b]           due: the bucket's due slots (counted into the bucket's backlog count, so the
//                                next inbox has room for their Terminated envelopes; read at the bucket's entry)
//   [kWdBucketOff + nb + b]      mark: a watch started in this bucket this tick (the end of the tick scans)
//   [kWdBucketOff + 2 * nb + b]  clock: the ticks bucket b has run (every bucket runs every tick: all equal)
//   [kWdBucketOff + 3 * nb + b]  nwatch: the bucket's watching slots
//   then, 16-byte aligned and slot-major ([slot][actor], np = nb << bb actors):
//     wee[slot][np]  the watchee id        st[slot][np]   state (free / watching / due / notified) | kWdHasMsg
//     gen[slot][np]  the generation        pay[slot][np]  the custom message
//   then died[np]: the actor's death tick, kWdNone while it is alive (written by the actor's own lane when it
//   stops, with an agent-scope relaxed store; 0 for an id that was never registered).
// Only a bucket's own block writes its actors' slots; died[] of other buckets is read at the end of a tick, and
// only values below the tick count: those were written in earlier launches.
constexpr uint32_t kWdBucketOff = 32;
constexpr uint32_t kWdLastAct = 2, kWdCtr = 4, kWdStopW = 14, kWdAnyW = 16, kWdFull = 18;
constexpr uint32_t kWdNone = 0xFFFFFFFFu, kWdGenMask = 0x3FFFFFu;
constexpr uint32_t kWdFree = 0, kWdWatching = 1, kWdDue = 2, kWdNotified = 3, kWdStateMask = 3, kWdHasMsg = 4;
constexpr uint32_t kWcWatches = 0, kWcTerminated = 1, kWcDiscarded = 2, kWcPacts = 3, kWcConflicts = 4;
__host__ __device__ __forceinline__ size_t wd_slot_off(uint32_t nb) {
  return ((size_t)kWdBucketOff + 4u * (size_t)nb + 3u) & ~(size_t)3;
}
struct WatchDev {
  uint32_t* base;
  uint32_t *wee, *st, *gen, *pay, *died;  // [slot * np + l]; died[l]
  uint32_t ns, np, nb, n;                 // n: the population (ids at or above it count as dead)
  __device__ __forceinline__ uint32_t* due(uint32_t b) const { return base + kWdBucketOff + b; }
  __device__ __forceinline__ uint32_t* mark(uint32_t b) const { return base + kWdBucketOff + nb + b; }
  __device__ __forceinline__ uint32_t& clock(uint32_t b) const { return base[kWdBucketOff + 2u * nb + b]; }
  __device__ __forceinline__ uint32_t* nwatch(uint32_t b) const { return base + kWdBucketOff + 3u * nb + b; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kWdCtr) + i;
  }
  __device__ __forceinline__ size_t at(uint32_t slot, uint32_t l) const { return (size_t)slot * np + l; }
  __device__ __forceinline__ uint32_t ld(const uint32_t* p) const {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void sto(uint32_t* p, uint32_t v) const {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // watch(x) / watchWith(x, m) by actor l of bucket b (DeathWatch.scala:23-47, checkWatchingSame :113): 0 = done
  // or a no-op, 1 = IllegalStateException; `slot_out`: the slot occupied now (ns: none)
  __device__ __forceinline__ uint32_t watch(uint32_t l, uint32_t b, uint32_t x, bool with, uint32_t m,
                                            uint32_t* slot_out = nullptr) const {
    if (slot_out) *slot_out = ns;
    if (x == l) return 0u;  // (single rank: the local id is the actor id)
    uint32_t fr = ns;
    for (uint32_t k = 0; k < ns; ++k) {
      const size_t i = at(k, l);
      const uint32_t s = st[i], state = s & kWdStateMask;
      if (state == kWdFree) {
        if (fr == ns) fr = k;
      } else if (wee[i] == x) {
        if (state == kWdNotified) return 0u;  // (the re-watch of a dead ref: its second Terminated would be dropped)
        const bool has = (s & kWdHasMsg) != 0u;
        return (has == with && (!with || pay[i] == m)) ? 0u : 1u;
      }
    }
    if (fr == ns) {  // no free slot: loud, the watch is not recorded
      sto(base + kWdFull, 1u);
      return 0u;
    }
    const size_t i = at(fr, l);
    wee[i] = x;
    st[i] = kWdWatching | (with ? kWdHasMsg : 0u);
    gen[i] = gen[i] + 1u;
    pay[i] = with ? m : 0u;
    atomicAdd(nwatch(b), 1u);
    sto(mark(b), 1u);
    atomicAdd(ctr(kWcWatches), 1ull);
    if (slot_out) *slot_out = fr;
    return 0u;
  }
  // unwatch(x): the slot holding x becomes free, in any state (DeathWatch.scala:49-60)
  __device__ __forceinline__ void unwatch(uint32_t l, uint32_t b, uint32_t x) const {
    for (uint32_t k = 0; k < ns; ++k) {
      const size_t i = at(k, l);
      const uint32_t state = st[i] & kWdStateMask;
      if (state != kWdFree && wee[i] == x) {
        if (state == kWdWatching) atomicSub(nwatch(b), 1u);
        st[i] = kWdFree;
      }
    }
  }
  // the actor stops in tick `now`: its slots become free (unwatchWatchedActors, :147-162), its death tick is set
  __device__ __forceinline__ void stop(uint32_t l, uint32_t b, uint32_t now) const {
    for (uint32_t k = 0; k < ns; ++k) {
      const size_t i = at(k, l);
      const uint32_t state = st[i] & kWdStateMask;
      if (state == kWdWatching) atomicSub(nwatch(b), 1u);
      if (state != kWdFree) st[i] = kWdFree;
    }
    sto(died + l, now);
    sto(base + kWdStopW + (now & 1u), now);
  }
  // is x dead before tick `now` (a death tick below it; an id outside the population always is)?
  __device__ __forceinline__ bool dead_before(uint32_t x, uint32_t now) const {
    if (x >= n) return true;
    const uint32_t d = ld(died + x);
    return d != kWdNone && d < now;
  }
};
// the third rule of "active at the entry of tick t": an actor stopped in tick t - 1 while a slot of the engine
// was watching at the end of t - 1 (both words were written in an earlier launch)
__device__ __forceinline__ bool wd_stop_seen(const uint32_t* base, uint32_t t) {
  const uint32_t p = t - 1u;
  return __hip_atomic_load(base + kWdStopW + (p & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p &&
         __hip_atomic_load(base + kWdAnyW + (p & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p;
}
__device__ __forceinline__ WatchDev watch_dev(uint32_t* base, uint32_t nb, uint32_t bb, uint32_t n) {
  WatchDev t;
  t.base = base;
  t.ns = base[0];
  t.nb = nb;
  t.np = nb << bb;
  t.n = n;
  t.wee = base + wd_slot_off(nb);
  t.st = t.wee + (size_t)t.ns * t.np;
  t.gen = t.st + (size_t)t.ns * t.np;
  t.pay = t.gen + (size_t)t.ns * t.np;
  t.died = t.pay + (size_t)t.ns * t.np;
  return t;
}

// ---- children (agx_set_children; AA/dungeon/Children.scala, TY/internal/adapter/
// ActorContextAdapter.scala:79-106).  An engine with death watch only.  The child storage is an allocation of its
// own; the watch storage's header words [kWdChildPtr, +2) hold its device address (0: no children).  u32 units:
//   [0] n_regions   [1] n_sites
//   [4..19]   eight u64 counters: spawned, refused, created, child_stops, cascade_stops, illegal_stops, discarded
//   [kCdRegionOff + 4 * r]  region r: first_parent, n_parents, first_child, max_children
//   [kCdSiteOff + 8 * s]    site s: kind, flags (kCdSiteParent: word 1 = the parent's id), word-0 base (lo, hi),
//                           word-1 constant (lo, hi)
//   [kCdBucketOff + b]      nlive: the bucket's live created children
//   then sc[np]: the actor's spawn count | kCdCreated once the actor was created by a Create envelope
// Only a bucket's own block writes its actors' words.  The k-th spawn of parent p creates id first_child +
// (p - first_parent) * max_children + k; the parent of an id is computed from the same formula.
constexpr uint32_t kWdChildPtr = 20;
constexpr uint32_t kCdCtr = 4, kCdRegionOff = 32, kCdSiteOff = 64, kCdBucketOff = kCdSiteOff + 8u * AGX_MAX_SPAWN_SITES;
constexpr uint32_t kCdCreated = 0x80000000u, kCdSiteParent = 1u;
constexpr uint32_t kCcSpawned = 0, kCcRefused = 1, kCcCreated = 2, kCcChildStops = 3, kCcCascade = 4, kCcIllegal = 5,
                   kCcDiscarded = 6;
__host__ __device__ __forceinline__ size_t cd_count_off(uint32_t nb) {
  return ((size_t)kCdBucketOff + (size_t)nb + 3u) & ~(size_t)3;
}
struct ChildDev {
  uint32_t* base;
  uint32_t* sc;  // [np]
  uint32_t nr, nsites;
  __device__ __forceinline__ uint32_t* nlive(uint32_t b) const { return base + kCdBucketOff + b; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kCdCtr) + i;
  }
  __device__ __forceinline__ const uint32_t* site(uint32_t s) const { return base + kCdSiteOff + 8u * s; }
  // the computed parent of id x (kWdNone: x lies in no child block)
  __device__ __forceinline__ uint32_t parent_of(uint32_t x) const {
    for (uint32_t r = 0; r < nr; ++r) {
      const uint32_t* R = base + kCdRegionOff + 4u * r;
      const uint32_t off = x - R[2];
      if (x >= R[2] && off < R[1] * R[3]) return R[0] + off / R[3];
    }
    return kWdNone;
  }
  // the child block of parent p: its first id and its size (false: p lies in no parent range)
  __device__ __forceinline__ bool block_of(uint32_t p, uint32_t& first, uint32_t& cap) const {
    for (uint32_t r = 0; r < nr; ++r) {
      const uint32_t* R = base + kCdRegionOff + 4u * r;
      const uint32_t off = p - R[0];
      if (p >= R[0] && off < R[1]) {
        first = R[2] + off * R[3];
        cap = R[3];
        return true;
      }
    }
    return false;
  }
  __device__ __forceinline__ uint32_t spawned(uint32_t l) const { return sc[l] & ~kCdCreated; }
  // context.spawn by actor l: the new child's id, or kWdNone when the spawn is refused
  __device__ __forceinline__ uint32_t spawn(uint32_t l) const {
    uint32_t first = 0, cap = 0;
    const uint32_t c = sc[l], n = c & ~kCdCreated;
    if (!block_of(l, first, cap) || n >= cap) {
      atomicAdd(ctr(kCcRefused), 1ull);
      return kWdNone;
    }
    sc[l] = c + 1u;
    atomicAdd(ctr(kCcSpawned), 1ull);
    return first + n;
  }
  // is x one of actor l's children already spawned?
  __device__ __forceinline__ bool own_child(uint32_t l, uint32_t x) const {
    uint32_t first = 0, cap = 0;
    if (!block_of(l, first, cap)) return false;
    return x >= first && x - first < spawned(l);
  }
  // child number i mod spawn count of actor l (kWdNone without children)
  __device__ __forceinline__ uint32_t child_at(uint32_t l, uint64_t i) const {
    uint32_t first = 0, cap = 0;
    const uint32_t n = spawned(l);
    if (!n || !block_of(l, first, cap)) return kWdNone;
    return first + (uint32_t)(i % n);
  }
};
__device__ __forceinline__ ChildDev child_dev(const uint32_t* watch_base, uint32_t nb) {
  ChildDev c;
  c.base = reinterpret_cast<uint32_t*>(*reinterpret_cast<const unsigned long long*>(watch_base + kWdChildPtr));
  c.nr = c.base[0];
  c.nsites = c.base[1];
  c.sc = c.base + cd_count_off(nb);
  return c;
}

// A tell to a host-side actor (agx_set_outbound): appended to the outbox (when `write`); returns
// false for any other id.  One thread's appends are ordered (same counter, program order), so each
// sender's outbound tells keep their emission order.
__device__ __forceinline__ bool outbound_tell(const DevParams& P, uint32_t dst, uint32_t src, uint32_t pay,
                                              bool write) {
  if (dst - P.host_lo >= P.host_n) return false;
  if (write) {
    // an append past outbox_cap is dropped and reported (then cleared) by agx_take_outbound from the
    // count itself -- not through the sticky error word, so the engine stays usable
    const uint32_t i = atomicAdd(P.outbox_n, 1u);
    if (i < P.outbox_cap) {
      P.outbox[3 * (size_t)i] = dst;
      P.outbox[3 * (size_t)i + 1] = src;
      P.outbox[3 * (size_t)i + 2] = pay;
    }
  }
  return true;
}

// ------------------------------------------------------------------ RNG
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t fanout_rand(uint64_t seed, uint32_t self, uint32_t h, uint32_t j) {
  return splitmix64(seed ^ splitmix64(((uint64_t)self << 32) ^ ((uint64_t)h << 4) ^ (uint64_t)j));
}
// First index i with cdf[i] >= u (clamped to n - 1), as a destination perm[i].  The top kZipfBits
// of u select an entry of the `zent` index built at agx_set_fanout: when every u of that range has
// the same answer i (the Zipf head: a hot destination spans many ranges) the entry holds perm[i]
// itself, {perm[i], kZipfDirect} -- one load in all; otherwise the search range {lo, hi} (lo = the
// answer for u = t << (32 - kZipfBits), hi = that of the next range, n - 1 after the last), a binary
// search over the CDF thresholds in it, then perm.  Same answer as the search over [0, n - 1].
constexpr uint32_t kZipfBits = 20;
constexpr uint32_t kZipfDirect = 0xFFFFFFFFu;  // (a range's hi is <= n - 1 < 2^32 - 1)
__device__ __forceinline__ uint32_t zipf_dest(const uint32_t* cdf, const uint32_t* perm, const uint2* zent, uint64_t r) {
  const uint32_t u = (uint32_t)(r >> 32);
  const uint2 z = zent[u >> (32 - kZipfBits)];
  if (z.y == kZipfDirect) return z.x;
  uint32_t lo = z.x, hi = z.y;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cdf[mid] >= u) hi = mid; else lo = mid + 1;
  }
  return perm[lo];
}

// ------------------------------------------------------------------ scans
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// inclusive wave64 sum scan over the whole (fully active) wave, in DPP: row_shr 1/2/4/8 scans each
// 16-lane row, row_bcast 15 / 31 carry the row totals into the rows above.  Six VALU ops with DPP
// operands instead of six ds_bpermute round trips through the LDS crossbar (__shfl_up): every
// block scan of the apply chain uses it.  (Lanes with no DPP source keep `old` = 0.)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ int wave_incl_max(int v) {
  const uint32_t lane = lane_id();
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    int t = __shfl_up(v, d, kWave);
    if (lane >= (uint32_t)d) v = max(v, t);
  }
  return v;
}

// Block exclusive sum over NT threads (NT multiple of 64, <= 1024).
// `scratch` needs NT/64 + 1 u32.  Returns exclusive prefix; *total = block sum.
// Two barriers: every thread sums the NT/64 wave totals itself (LDS broadcast reads) instead of
// one thread scanning them between two barriers.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t v, uint32_t* scratch, uint32_t* total) {
  constexpr int NW = NT / kWave;
  const int tid = threadIdx.x, w = tid / kWave, lane = tid % kWave;
  const uint32_t inc = wave_incl_sum(v);
  if (lane == kWave - 1) scratch[w] = inc;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t t = scratch[i];
    pre += i < w ? t : 0u;
    tot += t;
  }
  *total = tot;
  __syncthreads();  // (scratch is reused by the caller's next scan)
  return pre + inc - v;
}

// Two block exclusive sums at once (one set of barriers).  `scratch` needs 2 * (NT/64 + 1) u32.
template <int NT>
__device__ __forceinline__ uint2 block_excl_sum2(uint32_t v0, uint32_t v1, uint32_t* scratch, uint32_t* t0,
                                                 uint32_t* t1) {
  constexpr int NW = NT / kWave;
  const int tid = threadIdx.x, w = tid / kWave, lane = tid % kWave;
  const uint32_t i0 = wave_incl_sum(v0), i1 = wave_incl_sum(v1);
  if (lane == kWave - 1) {
    scratch[w] = i0;
    scratch[NW + 1 + w] = i1;
  }
  __syncthreads();
  uint32_t p0 = 0, p1 = 0, s0 = 0, s1 = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t a = scratch[i], b = scratch[NW + 1 + i];
    p0 += i < w ? a : 0u;
    p1 += i < w ? b : 0u;
    s0 += a;
    s1 += b;
  }
  *t0 = s0;
  *t1 = s1;
  __syncthreads();
  return make_uint2(p0 + i0 - v0, p1 + i1 - v1);
}

// Block exclusive max over NT threads; identity -1.
template <int NT>
__device__ __forceinline__ int block_excl_max(int v, int* scratch) {
  constexpr int NW = NT / kWave;
  const int tid = threadIdx.x, w = tid / kWave, lane = tid % kWave;
  int inc = wave_incl_max(v);
  int exc = __shfl_up(inc, 1, kWave);
  if (lane == 0) exc = -1;
  if (lane == kWave - 1) scratch[w] = inc;
  __syncthreads();
  if (tid == 0) {
    int run = -1;
    for (int i = 0; i < NW; ++i) { int t = scratch[i]; scratch[i] = run; run = max(run, t); }
  }
  __syncthreads();
  int r = max(scratch[w], exc);
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------ behaviours
// One ActorCell.invoke of one message (akka-actor/.../ActorCell.scala:539-555)
// through the typed ActorAdapter (TY/internal/adapter/ActorAdapter.scala:77-168).
// `Emit` is called for each tell: emit(dst_global, payload).
//
// KM is the set of behaviour kinds compiled in (bit k = kind k).  The engine
// launches the narrowest specialisation that covers every registered kind, so a
// population of one behaviour runs a small, branch-free apply kernel.
constexpr uint32_t kb(uint32_t k) { return 1u << (k < AGX_KIND_COMPILED ? k : AGX_KIND_COMPILED); }
// KM flag (not a kind): the variant runs delta-CRDT replication (agx_set_delta_crdt).  Variants
// without it compile the delta code out (its registers would spill the full-state merges).
constexpr uint32_t kDeltaKM = 1u << 31;
// KM flag (not a kind): the variant knows the stash of deque-based mailboxes (agx_set_stash).  A flag of KM,
// not a template parameter of its own, so every other instantiation keeps its name and compiles as before.
constexpr uint32_t kStashKM = 1u << 30;
// KM flag (not a kind): the variant knows timers (agx_set_timers).  A flag of KM for the same reason.
constexpr uint32_t kTimersKM = 1u << 29;
// KM flag (not a kind): the variant knows death watch (agx_set_death_watch).  A flag of KM for the same reason.
constexpr uint32_t kWatchKM = 1u << 28;
// KM flag (not a kind): the variant knows supervision (agx_set_supervision).  A flag of KM for the same reason.
constexpr uint32_t kSuperKM = 1u << 27;
// KM flag (not a kind): the variant knows children (agx_set_children); only ever combined with kWatchKM.
constexpr uint32_t kChildKM = 1u << 26;
// KM flag (not a kind): the variant knows receive timeouts (agx_set_receive_timeout); only ever combined with kTimersKM.
constexpr uint32_t kIdleKM = 1u << 25;
// KM flag (not a kind): the variant knows the receptionist (agx_set_receptionist).  A flag of KM for the same reason.
constexpr uint32_t kRecepKM = 1u << 24;
// KM flag (not a kind): the variant knows the ask pattern (agx_set_ask); only ever combined with kTimersKM.
constexpr uint32_t kAskKM = 1u << 23;
// KM flag (not a kind): the variant knows pub-sub topics (agx_set_topics); only ever combined with kRecepKM.
constexpr uint32_t kTopicKM = 1u << 22;
// KM flag (not a kind): the variant knows Subscribe / Listing (agx_set_listings); only ever with kRecepKM | kTopicKM.
constexpr uint32_t kListKM = 1u << 21;
// KM flag (not a kind): the variant knows consistent-hashing and random routing (agx_set_router_logics); only ever
// combined with kRecepKM.
constexpr uint32_t kHashKM = 1u << 20;
// KM flag (not a kind): the variant knows sharded entities (agx_set_sharding); only ever combined as
// kTimersKM | kIdleKM | kShardKM.
constexpr uint32_t kShardKM = 1u << 19;
// KM flag (not a kind): the variant knows restartWithBackoff (agx_set_backoff); only ever combined as
// kSuperKM | kBackoffKM.
constexpr uint32_t kBackoffKM = 1u << 18;
constexpr uint32_t KM_ALL = kb(AGX_KIND_COUNTER) | kb(AGX_KIND_RING) | kb(AGX_KIND_FANOUT) | kb(AGX_KIND_FORWARD_RR) |
                            kb(AGX_KIND_STOP_AFTER) | kb(AGX_KIND_PINGPONG) | kb(AGX_KIND_EVEN);

// ---- compiled behaviours (include/akka_gpu.h "compiled behaviours"; akka_amd/typed.py lowers them)
// (kStash: the stash instantiations know AGX_V_STASH, the size of the actor's stash buffer; every other
// instantiation compiles as before)
template <bool kStash = false>
__device__ __forceinline__ uint64_t cb_operand(uint32_t src, uint32_t word, int64_t k, uint32_t pay, const uint64_t* w,
                                               uint32_t sender, uint32_t self, uint32_t nstash = 0) {
  uint64_t b = 0;
  if constexpr (kStash)
    if (src == AGX_V_STASH) return (uint64_t)nstash + (uint64_t)k;
  switch (src) {
    case AGX_V_PAYLOAD: b = pay; break;
    case AGX_V_TAG: b = pay >> 24; break;
    case AGX_V_ARG: b = pay & 0xFFFFFFu; break;
    case AGX_V_WORD: b = w[word & 1u]; break;
    case AGX_V_SENDER: b = sender; break;
    case AGX_V_SELF: b = self; break;
    default: break;
  }
  return b + (uint64_t)k;
}
__device__ __forceinline__ bool cb_cmp(uint32_t op, uint64_t a, uint64_t b) {
  switch (op) {
    case AGX_CMP_EQ: return a == b;
    case AGX_CMP_NE: return a != b;
    case AGX_CMP_LT: return a < b;
    case AGX_CMP_LE: return a <= b;
    case AGX_CMP_GT: return a > b;
    case AGX_CMP_GE: return a >= b;
    default: return true;
  }
}
// ReceiveBuilder.receive (TY/javadsl/ReceiveBuilder.scala:209-218): the first case whose tests hold
template <bool kStash = false, typename Emit>
__device__ __forceinline__ uint32_t compiled_apply(const DevParams& P, uint32_t& kind, uint32_t self, uint64_t* w,
                                                uint32_t src, uint32_t pay, Emit& emit, uint32_t nstash = 0) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, cb_operand<kStash>(C.src1, C.word1, C.k1, pay, w, src, self, nstash),
                cb_operand<kStash>(C.src2, C.word2, C.k2, pay, w, src, self, nstash)))
      continue;
    if (!cb_cmp(C.cmp2, cb_operand<kStash>(C.src3, C.word3, C.k3, pay, w, src, self, nstash),
                cb_operand<kStash>(C.src4, C.word4, C.k4, pay, w, src, self, nstash)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = cb_operand<kStash>(A.src, A.sword, A.k, pay, w, src, self, nstash);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_TELL: {
          uint64_t d;
          if (A.dsrc == AGX_V_SELF) {  // (self + dk) mod n: ring neighbours
            int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
            d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
          } else {
            d = cb_operand<kStash>(A.dsrc, A.dword, A.dk, pay, w, src, self, nstash);
          }
          emit(d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d, A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v);
          break;
        }
        default: break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    if constexpr (kStash)  // unstash_all(next): the become here, the release by the caller
      if (C.result == AGX_RES_UNSTASH_ALL && C.next != AGX_NEXT_SAME) kind = AGX_KIND_COMPILED + C.next;
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// compiled_apply of the timer instantiations (agx_set_timers): the same rule, with AGX_V_TIMER
// (isTimerActive) among the operands and the timer actions, run in order with the others, against the
// actor's slots.  A function of its own: every other instantiation compiles compiled_apply as before.
__device__ __forceinline__ uint64_t tm_operand(const TimerDev& TD, uint32_t l, uint32_t src, uint32_t word, int64_t k,
                                               uint32_t pay, const uint64_t* w, uint32_t sender, uint32_t self) {
  if (src == AGX_V_TIMER)
    return (uint64_t)((word < TD.nk && (TD.per[TD.at(word, l)] & kTmActive)) ? 1u : 0u) + (uint64_t)k;
  return cb_operand(src, word, k, pay, w, sender, self);
}
// (kIdle: the receive-timeout instantiations, DESIGN.md §2.7 -- AGX_A_SET_RECEIVE_TIMEOUT / _CANCEL_ act on the
// actor's timeout in the caller's registers, `rt`; every other instantiation compiles as before)
// (kAsk: the ask instantiations, DESIGN.md §2.9 -- AGX_A_ASK_ARM starts the key as a single timer marked as an ask
// and leaves the ask ref in `ar`, AGX_A_ASK_SEND emits the case's one envelope with that ref as its sender; a plain
// timer start clears the mark.  `emit` is then an AskEmit)
// (kShard: the sharding instantiations, DESIGN.md §2.13 -- AGX_A_PASSIVATE only raises kRtPassivate in `rt`: the
// caller, which knows the entity's type and mark, sends the stop payload through the case's tell slot)
template <bool kIdle = false, bool kAsk = false, bool kShard = false, typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_tm(const DevParams& P, const TimerDev& TD, uint32_t l, uint32_t bkt,
                                                      uint32_t now, uint32_t& kind, uint32_t self, uint64_t* w,
                                                      uint32_t src, uint32_t pay, Emit& emit, RtRegs* rt = nullptr,
                                                      AskRegs* ar = nullptr) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, tm_operand(TD, l, C.src1, C.word1, C.k1, pay, w, src, self),
                tm_operand(TD, l, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, tm_operand(TD, l, C.src3, C.word3, C.k3, pay, w, src, self),
                tm_operand(TD, l, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = tm_operand(TD, l, A.src, A.sword, A.k, pay, w, src, self);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_TELL: {
          uint64_t d;
          if (A.dsrc == AGX_V_SELF) {  // (self + dk) mod n: ring neighbours
            int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
            d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
          } else {
            d = tm_operand(TD, l, A.dsrc, A.dword, A.dk, pay, w, src, self);
          }
          emit(d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d, A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v);
          break;
        }
        case AGX_A_TIMER_SINGLE:
        case AGX_A_TIMER_PERIODIC:
          if (A.word < TD.nk) {  // (a key past n_keys is refused at agx_run)
            TD.cancel(A.word, l, bkt);
            TD.start(A.word, l, bkt, now, tm_delay(tm_operand(TD, l, A.dsrc, A.dword, A.dk, pay, w, src, self)),
                     A.op == AGX_A_TIMER_PERIODIC, A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v);
            if constexpr (kAsk) ar->AD.row[TD.at(A.word, l)] = 0u;  // (no ask's timeout any more)
          }
          break;
        case AGX_A_TIMER_CANCEL:
          if (A.word < TD.nk) TD.cancel(A.word, l, bkt);
          break;
        case AGX_A_TIMER_CANCEL_ALL:
          for (uint32_t k = 0; k < TD.nk; ++k) TD.cancel(k, l, bkt);
          break;
        default:
          if constexpr (kIdle) {
            if (A.op == AGX_A_SET_RECEIVE_TIMEOUT) {
              rt->delay = tm_delay(tm_operand(TD, l, A.dsrc, A.dword, A.dk, pay, w, src, self));
              rt->pay = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
              rt->flags |= kRtChanged;
            } else if (A.op == AGX_A_CANCEL_RECEIVE_TIMEOUT) {
              rt->flags |= kRtChanged | (rt->delay ? kRtWasOff : 0u);
              rt->delay = 0u;
            }
          }
          if constexpr (kShard) {
            if (A.op == AGX_A_PASSIVATE) rt->flags |= kRtPassivate;
          }
          if constexpr (kAsk) {
            const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
            if (A.op == AGX_A_ASK_ARM) {
              if (A.word < TD.nk) {  // (a key past n_keys is refused at agx_run)
                TD.cancel(A.word, l, bkt);
                TD.start(A.word, l, bkt, now, tm_delay(tm_operand(TD, l, A.dsrc, A.dword, A.dk, pay, w, src, self)), false, msg);
                ar->AD.row[TD.at(A.word, l)] = kAskIs | ((A.pad0 & 1u) ? kAskHasTag | (uint32_t)A.pad1 : 0u);
                ar->ref = ask_ref(A.word, TD.agen[l], self);  // (start stored the slot's generation there)
                ++ar->cnt->c[kAcAsked];
              }
            } else if (A.op == AGX_A_ASK_SEND) {  // (directly after its ARM: agx_run refuses other tables)
              uint64_t d;
              if (A.dsrc == AGX_V_SELF) {  // (self + dk) mod n, as a TELL's
                int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
                d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
              } else {
                d = tm_operand(TD, l, A.dsrc, A.dword, A.dk, pay, w, src, self);
              }
              emit.send(ar->ref, d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d, msg);
            }
          }
          break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// compiled_apply of the death-watch instantiations (agx_set_death_watch): the same rule, with
// signal cases (AGX_CASE_SIGNAL in the result byte: an ordinary message skips them, a signal tries only them)
// and the watch actions, run in order with the others, against the actor's slots.  A watch that conflicts
// (checkWatchingSame) skips the rest of the case's actions and stops the actor: `conflict` is set and the
// result is AGX_RES_STOPPED.  A signal no case matches returns AGX_RES_UNHANDLED: the caller's death pact.
// A function of its own: every other instantiation compiles compiled_apply as before.
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_w(const DevParams& P, const WatchDev& WD, uint32_t l, uint32_t bkt,
                                                     uint32_t& kind, uint32_t self, uint64_t* w, uint32_t src,
                                                     uint32_t pay, bool signal, bool& conflict, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (((C.result & AGX_CASE_SIGNAL) != 0u) != signal) continue;
    if (!cb_cmp(C.cmp1, cb_operand(C.src1, C.word1, C.k1, pay, w, src, self),
                cb_operand(C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, cb_operand(C.src3, C.word3, C.k3, pay, w, src, self),
                cb_operand(C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = cb_operand(A.src, A.sword, A.k, pay, w, src, self);
      uint64_t d = 0;
      if (A.op == AGX_A_TELL || A.op >= AGX_A_WATCH) {  // a ref: (self + dk) mod n for ring neighbours
        if (A.dsrc == AGX_V_SELF) {
          int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
          d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
        } else {
          d = cb_operand(A.dsrc, A.dword, A.dk, pay, w, src, self);
        }
      }
      const uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_TELL: emit(ref, msg); break;
        case AGX_A_WATCH:
        case AGX_A_WATCH_WITH:
          if (WD.watch(l, bkt, ref, A.op == AGX_A_WATCH_WITH, msg)) {
            conflict = true;
            return AGX_RES_STOPPED;
          }
          break;
        case AGX_A_UNWATCH: WD.unwatch(l, bkt, ref); break;
        default: break;
      }
    }
    const uint32_t res = C.result & ~AGX_CASE_SIGNAL;
    if (res == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return res;
  }
  return AGX_RES_UNHANDLED;
}

// ---- supervision (agx_set_supervision; TY/internal/Supervision.scala:43-52,128-160,311-406)
// DevParams.super, u32 units:
//   [0]        n_levels: strategy entries per behaviour (1..4)
//   [1]        the behaviours the entry table covers
//   [2]        the clock's base: tick = clock + 1 - base (host-written after every run: a tick is a superstep
//              with mail, and the launches of a replay after quiescence advance the clocks, not the time)
//   [4..11]    four u64 counters: failures, resumes, restarts, stops
//   [kSvBucketOff + b]  clock: the launches bucket b has seen (every bucket sees every launch: all equal)
//   then, 16-byte aligned: the entries, AGX_MAX_SUPERVISORS per behaviour (agx_supervisor, 8 words each),
//   then level-major count[level][np] and deadline[level][np] (np = nb << bb actors; deadline 0: none),
//   then init_kind[np], one byte per actor: the kind the actor was registered with.
// Only an actor's own lane reads or writes its counts and deadlines, and only in sv_failed: a message that
// neither fails nor stops touches none of this.
constexpr uint32_t kSvBucketOff = 16;
constexpr uint32_t kSvLevels = 0, kSvBeh = 1, kSvBase = 2, kSvCtr = 4;
constexpr uint32_t kScFailures = 0, kScResumes = 1, kScRestarts = 2, kScStops = 3;
constexpr uint32_t kSvEntWords = AGX_MAX_BEHAVIORS * AGX_MAX_SUPERVISORS * 8u;
__host__ __device__ __forceinline__ size_t sv_ent_off(uint32_t nb) {
  return ((size_t)kSvBucketOff + (size_t)nb + 3u) & ~(size_t)3;
}
struct SuperDev {
  uint32_t* base;
  uint32_t nb, np;
  __device__ __forceinline__ uint32_t& clock(uint32_t b) const { return base[kSvBucketOff + b]; }
  __device__ __forceinline__ uint32_t tick(uint32_t b) const { return clock(b) + 1u - base[kSvBase]; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kSvCtr) + i;
  }
  __device__ __forceinline__ const agx_supervisor* entries(uint32_t beh) const {
    return reinterpret_cast<const agx_supervisor*>(base + sv_ent_off(nb)) + (size_t)beh * AGX_MAX_SUPERVISORS;
  }
  __device__ __forceinline__ uint32_t* count(uint32_t lev, uint32_t l) const {
    return base + sv_ent_off(nb) + kSvEntWords + (size_t)lev * np + l;
  }
  __device__ __forceinline__ uint32_t* deadline(uint32_t lev, uint32_t l) const {
    return count(base[kSvLevels] + lev, l);
  }
  __device__ __forceinline__ uint32_t init_kind(uint32_t l) const {
    return reinterpret_cast<const uint8_t*>(count(2u * base[kSvLevels], 0u))[l];
  }
};
__device__ __forceinline__ SuperDev super_dev(uint32_t* base, uint32_t nb, uint32_t bb) {
  return SuperDev{base, nb, nb << bb};
}

// compiled_apply of the children instantiations (agx_set_children): compiled_apply_w plus the
// operands AGX_V_SPAWNED / AGX_V_CHILD and the actions AGX_A_SPAWN / AGX_A_STOP_CHILD.  A spawn takes the next id
// of the actor's child block and tells it a Create envelope (the case's tell slot: max_emit is 1); a refused
// spawn sends nothing.  context.stop of a ref that is not one of the actor's spawned children is the reference's
// IllegalArgumentException: `illegal` is set, the rest of the case is skipped and the result is AGX_RES_STOPPED.
__device__ __forceinline__ uint64_t cc_operand(const ChildDev& CD, uint32_t l, uint32_t src, uint32_t word, int64_t k,
                                               uint32_t pay, const uint64_t* w, uint32_t sender, uint32_t self) {
  if (src == AGX_V_SPAWNED) return (uint64_t)CD.spawned(l) + (uint64_t)k;
  if (src == AGX_V_CHILD) return CD.child_at(l, (word <= 1u ? w[word] : 0ull) + (uint64_t)k);
  return cb_operand(src, word, k, pay, w, sender, self);
}
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_c(const DevParams& P, const WatchDev& WD, const ChildDev& CD, uint32_t l,
                                                     uint32_t bkt, uint32_t& kind, uint32_t self, uint64_t* w, uint32_t src,
                                                     uint32_t pay, bool signal, bool& conflict, bool& illegal, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (((C.result & AGX_CASE_SIGNAL) != 0u) != signal) continue;
    if (!cb_cmp(C.cmp1, cc_operand(CD, l, C.src1, C.word1, C.k1, pay, w, src, self),
                cc_operand(CD, l, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, cc_operand(CD, l, C.src3, C.word3, C.k3, pay, w, src, self),
                cc_operand(CD, l, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = cc_operand(CD, l, A.src, A.sword, A.k, pay, w, src, self);
      uint64_t d = 0;
      if (A.op == AGX_A_TELL || (A.op >= AGX_A_WATCH && A.op != AGX_A_SPAWN)) {  // a ref
        if (A.dsrc == AGX_V_SELF) {
          int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
          d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
        } else {
          d = cc_operand(CD, l, A.dsrc, A.dword, A.dk, pay, w, src, self);
        }
      }
      const uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_TELL: emit(ref, msg); break;
        case AGX_A_WATCH:
        case AGX_A_WATCH_WITH:
          if (WD.watch(l, bkt, ref, A.op == AGX_A_WATCH_WITH, msg)) {
            conflict = true;
            return AGX_RES_STOPPED;
          }
          break;
        case AGX_A_UNWATCH: WD.unwatch(l, bkt, ref); break;
        case AGX_A_SPAWN: {  // dword: the site; pad0 & 1: state word `word` receives the child's id
          const uint32_t ch = CD.spawn(l);
          if (A.pad0 & 1u) w[A.word & 1u] = ch;
          if (ch != kWdNone)
            emit(ch, (AGX_TAG_CREATE << 24) | (((uint32_t)A.dword & (AGX_MAX_SPAWN_SITES - 1u)) << AGX_SPAWN_ARG_BITS) |
                         ((uint32_t)v & AGX_SPAWN_ARG_MASK));
          break;
        }
        case AGX_A_STOP_CHILD:
          if (!CD.own_child(l, ref)) {
            illegal = true;
            return AGX_RES_STOPPED;
          }
          emit(ref, AGX_TAG_STOP << 24);
          break;
        default: break;
      }
    }
    const uint32_t res = C.result & ~AGX_CASE_SIGNAL;
    if (res == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return res;
  }
  return AGX_RES_UNHANDLED;
}

// compiled_apply of the supervision instantiations (agx_set_supervision): the same rule, with
// signal cases (an ordinary message skips them, a signal tries only them) and the result AGX_RES_FAIL, whose
// exception class (agx_case.next) is returned in `cls`.  A function of its own: every other instantiation
// compiles compiled_apply as before.
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_s(const DevParams& P, uint32_t& kind, uint32_t self, uint64_t* w,
                                                     uint32_t src, uint32_t pay, bool signal, uint32_t& cls, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (((C.result & AGX_CASE_SIGNAL) != 0u) != signal) continue;
    if (!cb_cmp(C.cmp1, cb_operand(C.src1, C.word1, C.k1, pay, w, src, self),
                cb_operand(C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, cb_operand(C.src3, C.word3, C.k3, pay, w, src, self),
                cb_operand(C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = cb_operand(A.src, A.sword, A.k, pay, w, src, self);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_TELL: {
          uint64_t d;
          if (A.dsrc == AGX_V_SELF) {  // (self + dk) mod n: ring neighbours
            int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
            d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
          } else {
            d = cb_operand(A.dsrc, A.dword, A.dk, pay, w, src, self);
          }
          emit(d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d, A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v);
          break;
        }
        default: break;
      }
    }
    const uint32_t res = C.result & ~AGX_CASE_SIGNAL;
    if (res == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    if (res == AGX_RES_FAIL) cls = C.next;
    return res;
  }
  return AGX_RES_UNHANDLED;
}

// The cold path of the supervision drain: message handling of actor l (bucket b) ended in `res`, AGX_RES_FAIL of
// exception class `cls` or AGX_RES_STOPPED.  Returns AGX_RES_SAME (resumed or restarted: the drain goes on, `kind`
// and `w` are the actor's behaviour and state from here) or AGX_RES_STOPPED (PostStop has run).  Not inlined:
// the common drain's register use must not grow by this.
template <typename Emit>
__device__ __noinline__ uint32_t sv_failed(const DevParams& P, uint32_t nb, uint32_t bb, uint32_t l, uint32_t b,
                                           uint32_t& kind, uint32_t self, uint64_t* w, uint32_t res, uint32_t cls,
                                           Emit& emit) {
  const SuperDev SV = super_dev(P.super, nb, bb);
  uint32_t none = 0;
  if (res == AGX_RES_FAIL) {
    atomicAdd(SV.ctr(kScFailures), 1ull);
    const uint32_t ik = SV.init_kind(l), ib = ik - AGX_KIND_COMPILED, nl = SV.base[kSvLevels];
    if (ik >= AGX_KIND_COMPILED && ib < SV.base[kSvBeh]) {
      const agx_supervisor* const E = SV.entries(ib);
      const uint32_t t = SV.tick(b);
      for (uint32_t lev = 0; lev < nl; ++lev) {  // inner first
        if (!((E[lev].class_mask >> (cls & 31u)) & 1u)) continue;
        const uint32_t strat = E[lev].strategy;
        if (strat == AGX_SUP_RESUME) {
          atomicAdd(SV.ctr(kScResumes), 1ull);
          return AGX_RES_SAME;
        }
        if (strat != AGX_SUP_RESTART) break;  // STOP
        const uint32_t c = *SV.count(lev, l), d = *SV.deadline(lev, l);
        const bool left = d == 0u || t <= d;
        const int32_t mx = E[lev].max_restarts;
        if (mx != -1 && c >= (uint32_t)mx && left) continue;  // rethrown: the next outer entry that catches it
        if (kind >= AGX_KIND_COMPILED) compiled_apply_s(P, kind, self, w, self, AGX_SIGNAL_PRERESTART, true, none, emit);
        *SV.count(lev, l) = left ? c + 1u : 1u;
        *SV.deadline(lev, l) = (d != 0u && left) ? d : t + E[lev].within;
        for (uint32_t in = 0; in < lev; ++in) {  // a restart re-creates the inner interceptors
          *SV.count(in, l) = 0u;
          *SV.deadline(in, l) = 0u;
        }
        kind = ik;
        if (E[lev].reset_mask & 1u) w[0] = E[lev].reset[0];
        if (E[lev].reset_mask & 2u) w[1] = E[lev].reset[1];
        atomicAdd(SV.ctr(kScRestarts), 1ull);
        return AGX_RES_SAME;
      }
    }
  }
  if (kind >= AGX_KIND_COMPILED) compiled_apply_s(P, kind, self, w, self, AGX_SIGNAL_POSTSTOP, true, none, emit);
  atomicAdd(SV.ctr(kScStops), 1ull);
  return AGX_RES_STOPPED;
}

// ---- restartWithBackoff (agx_set_backoff; TY/internal/Supervision.scala:163-406), on top of
// supervision.  An allocation of its own, reached from words kSvBackoff, kSvBackoff + 1 of the SuperDev header
// (its address), u32 units:
//   [0]      n_levels (agx_set_supervision's)
//   [4..9]   three u64 counters: backoffs, dropped, limit_stops
//   [kBoBucketOff + b]  bound: the largest `until` any actor of bucket b was given (atomicMax at the failure): a
//            bucket whose bound is at or before the tick holds no suspended actor
//   then, 16-byte aligned: the rows, AGX_MAX_SUPERVISORS per behaviour, kBoRowWords words each (agx_backoff first),
//   then until[np] (the first tick at which the actor drains again; 0: never suspended), cap[np] (the stash bound of
//   its suspension, kBoNoBound: none of its own) and cut[np] (kBoCut | the index of the first message held, written
//   by the drain at the failure and cleared by bo_requeue in the same tick).
// A backoff entry keeps its reset-due in the entry's deadline word (SuperDev), which it does not use otherwise.
// Only an actor's own lane writes its words, and only on the cold path.
constexpr uint32_t kSvBackoff = 12;
constexpr uint32_t kBoCtr = 4, kBoBucketOff = 16, kBoRowWords = 8;
constexpr uint32_t kBcBackoffs = 0, kBcDropped = 1, kBcLimitStops = 2;
constexpr uint32_t kBoCut = 0x80000000u, kBoNoBound = 0xFFFFFFFFu;
constexpr uint32_t kBoSuspended = 0x100u;  // bo_failed's third answer: restarted, and suspended from the next message on
constexpr uint32_t kBoAlive = 0x80u;       // LDS alive byte, bit 7: the actor is suspended in this tick (bo_classify)
__host__ __device__ __forceinline__ size_t bo_row_off(uint32_t nb) {
  return ((size_t)kBoBucketOff + (size_t)nb + 3u) & ~(size_t)3;
}
__host__ __device__ __forceinline__ size_t bo_until_off(uint32_t nb) {
  return bo_row_off(nb) + (size_t)AGX_MAX_BEHAVIORS * AGX_MAX_SUPERVISORS * kBoRowWords;
}
struct BackoffDev {
  uint32_t* base;
  uint32_t nb, np;
  __device__ __forceinline__ uint32_t* bound(uint32_t b) const { return base + kBoBucketOff + b; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kBoCtr) + i;
  }
  __device__ __forceinline__ const agx_backoff* row(uint32_t beh, uint32_t lev) const {
    return reinterpret_cast<const agx_backoff*>(base + bo_row_off(nb) + ((size_t)beh * AGX_MAX_SUPERVISORS + lev) * kBoRowWords);
  }
  __device__ __forceinline__ uint32_t* until(uint32_t l) const { return base + bo_until_off(nb) + l; }
  __device__ __forceinline__ uint32_t* cap(uint32_t l) const { return until(l) + np; }
  __device__ __forceinline__ uint32_t* cut(uint32_t l) const { return until(l) + 2u * (size_t)np; }
};
__device__ __forceinline__ BackoffDev backoff_dev(const uint32_t* super, uint32_t nb, uint32_t bb) {
  const uint64_t p = (uint64_t)super[kSvBackoff] | ((uint64_t)super[kSvBackoff + 1u] << 32);
  return BackoffDev{reinterpret_cast<uint32_t*>(p), nb, nb << bb};
}

// sv_failed of the backoff instantiations: the same catch clause, with the entries that carry a backoff row (rules
// 1-5 of §2.14).  Returns AGX_RES_SAME, AGX_RES_STOPPED or kBoSuspended (restarted: `kind` and `w` are the re-created
// behaviour and state; the drain's window ends at this message and `until`, the stash bound and the bucket's bound
// are written).  A function of its own: the supervision instantiations compile sv_failed as before.  Not inlined.
template <typename Emit>
__device__ __noinline__ uint32_t bo_failed(const DevParams& P, uint32_t nb, uint32_t bb, uint32_t l, uint32_t b,
                                           uint32_t& kind, uint32_t self, uint64_t* w, uint32_t res, uint32_t cls,
                                           Emit& emit) {
  const SuperDev SV = super_dev(P.super, nb, bb);
  const BackoffDev BD = backoff_dev(P.super, nb, bb);
  uint32_t none = 0;
  if (res == AGX_RES_FAIL) {
    atomicAdd(SV.ctr(kScFailures), 1ull);
    const uint32_t ik = SV.init_kind(l), ib = ik - AGX_KIND_COMPILED, nl = SV.base[kSvLevels];
    if (ik >= AGX_KIND_COMPILED && ib < SV.base[kSvBeh]) {
      const agx_supervisor* const E = SV.entries(ib);
      const uint32_t t = SV.tick(b);
      for (uint32_t lev = 0; lev < nl; ++lev) {  // inner first
        if (!((E[lev].class_mask >> (cls & 31u)) & 1u)) continue;
        const uint32_t strat = E[lev].strategy;
        if (strat == AGX_SUP_RESUME) {
          atomicAdd(SV.ctr(kScResumes), 1ull);
          return AGX_RES_SAME;
        }
        if (strat != AGX_SUP_RESTART) break;  // STOP
        const agx_backoff R = *BD.row(ib, lev);
        uint32_t c = *SV.count(lev, l), d = *SV.deadline(lev, l);
        const int32_t mx = E[lev].max_restarts;
        if (R.min_backoff == 0u) {  // a plain restart: sv_failed's rule
          const bool left = d == 0u || t <= d;
          if (mx != -1 && c >= (uint32_t)mx && left) continue;  // rethrown: the next outer entry that catches it
          if (kind >= AGX_KIND_COMPILED) compiled_apply_s(P, kind, self, w, self, AGX_SIGNAL_PRERESTART, true, none, emit);
          *SV.count(lev, l) = left ? c + 1u : 1u;
          *SV.deadline(lev, l) = (d != 0u && left) ? d : t + E[lev].within;
        } else {
          if (d != 0u && t >= d) {  // ResetRestartCount(current), lazily: the reset-due has passed
            c = d = 0u;
            *SV.count(lev, l) = 0u;
            *SV.deadline(lev, l) = 0u;
          }
          if (mx != -1 && c >= (uint32_t)mx) {  // BehaviorImpl.failed (:314-320): not rethrown
            atomicAdd(BD.ctr(kBcLimitStops), 1ull);
            break;
          }
          if (kind >= AGX_KIND_COMPILED) compiled_apply_s(P, kind, self, w, self, AGX_SIGNAL_PRERESTART, true, none, emit);
          *SV.count(lev, l) = c + 1u;
          // calculateDelay (:163-173) in 64-bit integers: delay < 2^31, the factors < 2^17 and 2^16
          uint64_t delay = (uint64_t)R.min_backoff << (c >= 30u ? 0u : c);
          if (c >= 30u || delay > (uint64_t)R.max_backoff) delay = R.max_backoff;
          const uint64_t r16 = fanout_rand(P.fan_seed, self, t, 0u) >> 48;
          delay += (delay * (uint64_t)R.random_factor_q16 * r16) >> 32;
          const uint64_t until = (uint64_t)t + delay > 0xFFFFFFFFull ? 0xFFFFFFFFull : (uint64_t)t + delay;
          const uint64_t due = until + (uint64_t)R.reset_after > 0xFFFFFFFFull ? 0xFFFFFFFFull : until + (uint64_t)R.reset_after;
          *BD.until(l) = (uint32_t)until;
          *SV.deadline(lev, l) = (uint32_t)due;
          uint32_t C, T;
          mbox_limits(P, P.alive[l], C, T);
          *BD.cap(l) = R.stash_capacity >= 0 ? (uint32_t)R.stash_capacity : (C ? C : kBoNoBound);
          atomicMax(BD.bound(b), (uint32_t)until);
          atomicAdd(BD.ctr(kBcBackoffs), 1ull);
        }
        for (uint32_t in = 0; in < lev; ++in) {  // a restart re-creates the inner interceptors
          *SV.count(in, l) = 0u;
          *SV.deadline(in, l) = 0u;
        }
        kind = ik;
        if (E[lev].reset_mask & 1u) w[0] = E[lev].reset[0];
        if (E[lev].reset_mask & 2u) w[1] = E[lev].reset[1];
        atomicAdd(SV.ctr(kScRestarts), 1ull);
        return R.min_backoff == 0u ? AGX_RES_SAME : kBoSuspended;
      }
    }
  }
  if (kind >= AGX_KIND_COMPILED) compiled_apply_s(P, kind, self, w, self, AGX_SIGNAL_POSTSTOP, true, none, emit);
  atomicAdd(SV.ctr(kScStops), 1ull);
  return AGX_RES_STOPPED;
}

// ---- the receptionist and group routers (agx_set_receptionist; TY/internal/receptionist/
// LocalReceptionist.scala:147-248, TY/internal/routing/GroupRouterImpl.scala:114-146, RoutingLogic.scala:42-75).
// DevParams.recep, an allocation of its own, u32 units:
//   [0] n_keys   [1] capacity   [2] nb
//   [3] flags: bit k = key k changed in the tick being drained (dirty, OR-ed by the drains); bit 8 + k = key k is
//       being rebuilt (dirty_now: k_recep_scan moves the bit there, k_recep_fill reads it)
//   [8..19]  six u64 counters: routed, no_routees, registered, deregistered, terminated, rebuilds
//   [24..31] size[k] of the listing in force   [32..47] eight u64 version[k]
//   [kRcCntOff + k * nb + b]  cnt: the members of key k in bucket b (written by the bucket's own block)
//   then off[k * nb + b]: their offset in the listing (k_recep_scan), then list[k * capacity + i]: the listing of
//   key k, ascending ids (k_recep_fill), then one mask byte per actor (nb << bb of them): bit k = registered
// Only an actor's own lane writes its mask byte; the listings are written between two applies only.
constexpr uint32_t kRcFlags = 3, kRcCtr = 8, kRcSize = 24, kRcVersion = 32, kRcCntOff = 64;
constexpr uint32_t kRcRouted = 0, kRcNoRoutees = 1, kRcRegistered = 2, kRcDeregistered = 3, kRcTerminated = 4, kRcRebuilds = 5;
constexpr uint32_t kRcNone = 0xFFFFFFFFu;
__host__ __device__ __forceinline__ size_t rc_list_off(uint32_t nk, uint32_t nb) { return (size_t)kRcCntOff + 2ull * nk * nb; }
__host__ __device__ __forceinline__ size_t rc_mask_off(uint32_t nk, uint32_t cap, uint32_t nb) {
  return (rc_list_off(nk, nb) + (size_t)nk * cap + 3u) & ~(size_t)3;
}
struct RecepDev {
  uint32_t* base;
  uint8_t* mask;  // [nb << bb]
  uint32_t nk, cap, nb;
  __device__ __forceinline__ uint32_t* cnt(uint32_t k, uint32_t b) const { return base + kRcCntOff + (size_t)k * nb + b; }
  __device__ __forceinline__ uint32_t* off(uint32_t k, uint32_t b) const { return base + kRcCntOff + (size_t)(nk + k) * nb + b; }
  __device__ __forceinline__ uint32_t* list(uint32_t k) const { return base + rc_list_off(nk, nb) + (size_t)k * cap; }
  __device__ __forceinline__ uint32_t size(uint32_t k) const { return k < nk ? base[kRcSize + k] : 0u; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kRcCtr) + i;
  }
  // listing[x mod size] of key k (none: an empty listing)
  __device__ __forceinline__ uint32_t at(uint32_t k, uint64_t x) const {
    const uint32_t n = size(k);
    return n ? list(k)[(uint32_t)(x % n)] : kRcNone;
  }
  // round robin: the smallest listed id >= cursor, else listing[0] (none: an empty listing)
  __device__ __forceinline__ uint32_t successor(uint32_t k, uint64_t cursor) const {
    const uint32_t n = size(k);
    if (!n) return kRcNone;
    const uint32_t* const ls = list(k);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((uint64_t)ls[mid] < cursor) lo = mid + 1u;
      else hi = mid;
    }
    return ls[lo == n ? 0u : lo];
  }
};
__device__ __forceinline__ RecepDev recep_dev(uint32_t* base) {
  RecepDev r;
  r.base = base;
  r.nk = base[0];
  r.cap = base[1];
  r.nb = base[2];
  r.mask = reinterpret_cast<uint8_t*>(base + rc_mask_off(r.nk, r.cap, r.nb));
  return r;
}
// what one thread's drains changed: counted in registers, added to the storage once per wave (recep_commit)
struct RecepCount {
  uint32_t routed, none, reg, dereg, term, chg;  // chg: the key bits that differ over an actor's window
};

// compiled_apply of the receptionist instantiations: compiled_apply plus the operands AGX_V_LISTING_SIZE /
// AGX_V_SERVICE_AT and the actions AGX_A_REGISTER / AGX_A_DEREGISTER / AGX_A_ROUTE, against the actor's mask byte
// `mk` (a register of the drain) and the listings in force.  A forward (AGX_ROUTE_KEEP_SENDER) emits with the
// emitter's `self` replaced by the message's sender for that one call.  A function of its own: every other
// instantiation compiles compiled_apply as before.
// (compiled_apply_rc's cases are copied into compiled_apply_tp and compiled_apply_ls below: a fix to the set, tell,
// route or register cases belongs in all three.)
__device__ __forceinline__ uint64_t rc_operand(const RecepDev& RD, uint32_t src, uint32_t word, int64_t k, uint32_t pay,
                                               const uint64_t* w, uint32_t sender, uint32_t self) {
  if (src == AGX_V_LISTING_SIZE) return (uint64_t)RD.size(word & 7u) + (uint64_t)k;
  if (src == AGX_V_SERVICE_AT) {
    const uint32_t sel = (word >> 3) & 3u;
    const uint64_t x = sel <= AGX_SVC_WORD1 ? w[sel] : sel == AGX_SVC_ARG ? (uint64_t)(pay & 0xFFFFFFu) : 0ull;
    return RD.at(word & 7u, x + (uint64_t)k);
  }
  return cb_operand(src, word, k, pay, w, sender, self);
}
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_rc(const DevParams& P, const RecepDev& RD, uint32_t& kind, uint32_t self,
                                                      uint64_t* w, uint32_t src, uint32_t pay, uint32_t& mk, RecepCount& rc,
                                                      Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, rc_operand(RD, C.src1, C.word1, C.k1, pay, w, src, self),
                rc_operand(RD, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, rc_operand(RD, C.src3, C.word3, C.k3, pay, w, src, self),
                rc_operand(RD, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = rc_operand(RD, A.src, A.sword, A.k, pay, w, src, self);
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      const uint32_t bit = 1u << (A.pad1 & 7u);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_REGISTER:
          if (!(mk & bit)) {
            mk |= bit;
            ++rc.reg;
          }
          break;
        case AGX_A_DEREGISTER:
          if (mk & bit) {
            mk &= ~bit;
            ++rc.dereg;
          }
          break;
        case AGX_A_TELL:
        case AGX_A_ROUTE: {
          uint64_t d = 0;
          if (A.op == AGX_A_TELL || (A.pad0 & AGX_ROUTE_BY_INDEX)) {
            if (A.dsrc == AGX_V_SELF && A.op == AGX_A_TELL) {  // (self + dk) mod n: ring neighbours
              int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
              d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
            } else {
              d = rc_operand(RD, A.dsrc, A.dword, A.dk, pay, w, src, self);
            }
          }
          uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
          if (A.op == AGX_A_ROUTE) {
            const uint32_t key = A.pad1 & 7u;
            if (A.pad0 & AGX_ROUTE_BY_INDEX) {
              ref = RD.at(key, d);
            } else {
              ref = RD.successor(key, w[A.word & 1u]);
              if (ref != kRcNone) w[A.word & 1u] = (uint64_t)ref + 1ull;  // (no routee: the cursor stays)
            }
            if (ref == kRcNone) ++rc.none;
            else ++rc.routed;
          }
          if (A.pad0 & AGX_ROUTE_KEEP_SENDER) {  // a forward: the envelope keeps the incoming message's sender
            const uint32_t me = emit.self;
            emit.self = src;
            emit(ref, msg);
            emit.self = me;
          } else {
            emit(ref, msg);
          }
          break;
        }
        default: break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// ---- pub-sub topics (agx_set_topics; TY/internal/pubsub/TopicImpl.scala:60-143), on top of the
// receptionist: a topic is a service key, its subscribers are the key's registered actors.  An allocation of its
// own whose address stands in words [kRcTopicPtr, kRcTopicPtr + 2) of the receptionist's storage, u32 units:
//   [0] log_capacity   [1] nb
//   [4] cursor: the publications staged by the drains of the tick being drained   [5] mail: a bucket had mail in
//       this superstep (it is a tick)   [6] n_log: the entries of the pending log   (one 16-byte load: k_topic_plan)
//   [8..15]  four u64 counters: published, fanned_out, no_subscribers, host_published
//   [16..19] two u64: what the pending log added to fanned_out / no_subscribers (a re-plan takes it back)
//   [24..31] pubs[k]: the pending log's publications per key
//   [kTpDueOff + b]  due: the deliveries of the pending log to bucket b, part of the bucket's backlog count
//   then log[i] (uint4: key, sender, payload, 0), log_capacity entries: the publications the next tick delivers,
//   device publications in (publisher, window index) order, then host publications in call order
//   then stage[i] (uint4: publisher, window index, key, payload), log_capacity entries, in no order
// The drains only append to `stage`; k_topic_plan (after the apply) turns it into the log; the blocks of the next
// apply read the log, their own due word and their own mask bytes.
constexpr uint32_t kRcTopicPtr = 4;
constexpr uint32_t kTpCursor = 4, kTpMail = 5, kTpNLog = 6, kTpCtr = 8, kTpLast = 16, kTpPubs = 24, kTpDueOff = 32;
constexpr uint32_t kTpPublished = 0, kTpFannedOut = 1, kTpNoSubscribers = 2, kTpHostPublished = 3;
constexpr uint32_t kTpDueMax = 1u << 20;  // (a due count above one tile is an error either way: no 32-bit overflow)
__host__ __device__ __forceinline__ size_t tp_log_off(uint32_t nb) { return ((size_t)kTpDueOff + nb + 3u) & ~(size_t)3; }
__host__ __device__ __forceinline__ size_t tp_stage_off(uint32_t cap, uint32_t nb) { return tp_log_off(nb) + 4ull * cap; }
__host__ __device__ __forceinline__ size_t tp_words(uint32_t cap, uint32_t nb) { return tp_stage_off(cap, nb) + 4ull * cap; }
struct TopicDev {
  uint32_t* base;
  uint32_t cap, nb;
  __device__ __forceinline__ uint32_t* due(uint32_t b) const { return base + kTpDueOff + b; }
  __device__ __forceinline__ uint4* log() const { return reinterpret_cast<uint4*>(base + tp_log_off(nb)); }
  __device__ __forceinline__ uint4* stage() const { return reinterpret_cast<uint4*>(base + tp_stage_off(cap, nb)); }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kTpCtr) + i;
  }
  __device__ __forceinline__ unsigned long long* last(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kTpLast) + i;
  }
};
__device__ __forceinline__ TopicDev topic_dev(uint32_t* base) {
  TopicDev t;
  t.base = base;
  t.cap = base[0];
  t.nb = base[1];
  return t;
}
__device__ __forceinline__ TopicDev topic_dev_of(const uint32_t* recep) {
  return topic_dev(*reinterpret_cast<uint32_t* const*>(recep + kRcTopicPtr));
}

// compiled_apply of the topic instantiations: compiled_apply_rc plus AGX_A_PUBLISH, which appends (publisher, index
// within the publisher's drained window `q`, key, payload) to the tick's staging area and does not touch the
// emitter; an entry past log_capacity is not stored (k_topic_plan raises the error from the cursor).  `npub`: the
// thread's publish actions, added to the counter once per wave (topic_commit).  A function of its own: every other
// instantiation compiles compiled_apply_rc as before.
// (The set / tell / route / register / publish cases stand in three copies: compiled_apply_rc, this one and
// compiled_apply_ls.  A fix to one of them belongs in all three.)
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_tp(const DevParams& P, const RecepDev& RD, const TopicDev& TP, uint32_t& kind,
                                                      uint32_t self, uint64_t* w, uint32_t src, uint32_t pay, uint32_t& mk,
                                                      RecepCount& rc, uint32_t q, uint32_t& npub, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, rc_operand(RD, C.src1, C.word1, C.k1, pay, w, src, self),
                rc_operand(RD, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, rc_operand(RD, C.src3, C.word3, C.k3, pay, w, src, self),
                rc_operand(RD, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = rc_operand(RD, A.src, A.sword, A.k, pay, w, src, self);
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      const uint32_t bit = 1u << (A.pad1 & 7u);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_REGISTER:
          if (!(mk & bit)) {
            mk |= bit;
            ++rc.reg;
          }
          break;
        case AGX_A_DEREGISTER:
          if (mk & bit) {
            mk &= ~bit;
            ++rc.dereg;
          }
          break;
        case AGX_A_PUBLISH: {
          const uint32_t slot = atomicAdd(TP.base + kTpCursor, 1u);
          if (slot < TP.cap) TP.stage()[slot] = make_uint4(self, q, A.pad1 & 7u, msg);
          ++npub;
          break;
        }
        case AGX_A_TELL:
        case AGX_A_ROUTE: {
          uint64_t d = 0;
          if (A.op == AGX_A_TELL || (A.pad0 & AGX_ROUTE_BY_INDEX)) {
            if (A.dsrc == AGX_V_SELF && A.op == AGX_A_TELL) {  // (self + dk) mod n: ring neighbours
              int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
              d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
            } else {
              d = rc_operand(RD, A.dsrc, A.dword, A.dk, pay, w, src, self);
            }
          }
          uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
          if (A.op == AGX_A_ROUTE) {
            const uint32_t key = A.pad1 & 7u;
            if (A.pad0 & AGX_ROUTE_BY_INDEX) {
              ref = RD.at(key, d);
            } else {
              ref = RD.successor(key, w[A.word & 1u]);
              if (ref != kRcNone) w[A.word & 1u] = (uint64_t)ref + 1ull;  // (no routee: the cursor stays)
            }
            if (ref == kRcNone) ++rc.none;
            else ++rc.routed;
          }
          if (A.pad0 & AGX_ROUTE_KEEP_SENDER) {  // a forward: the envelope keeps the incoming message's sender
            const uint32_t me = emit.self;
            emit.self = src;
            emit(ref, msg);
            emit.self = me;
          } else {
            emit(ref, msg);
          }
          break;
        }
        default: break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// ---- Receptionist.Subscribe / Find and the Listing message (agx_set_listings; TY/internal/
// receptionist/LocalReceptionist.scala:152-171,209-220,233-238), on top of topics.  An allocation of its own whose
// address stands in words [kRcListPtr, kRcListPtr + 2) of the receptionist's storage, u32 units:
//   [0] n_keys   [1] nb   [2] bb
//   [4] mail: a bucket had mail in this superstep (it is a tick)   [5] changed: bit k = the Listings of the next
//       tick announce a change of key k   [6] pend: a pending bit was set since the last plan   [7] planned: the
//       standing plan holds deliveries (words [16..19] are not zero)   (one 16-byte load: k_listing_plan)
//   [8..15]  four u64 counters: subscribes, finds, listings_sent, notified
//   [16..19] two u64: what the standing plan added to listings_sent / notified (a re-plan takes it back)
//   [24..31] payload[k]: the payload of a Listing envelope of key k
//   [32..47] eight u64 seen[k]: the version of key k at the start of the host's calls between two runs (a key whose
//       version differs at their end was changed by them: the re-plan adds it to `changed` once)
//   [kLsDueOff + b]  due: the Listings planned for bucket b, part of the bucket's backlog count
//   then cnt_u[k * nb + b]: the actors of bucket b with bit k of sub | pending, then cnt_p[k * nb + b]: with bit k of
//   pending (both written by the bucket's own block), then one `sub` byte per actor (nb << bb of them), then one
//   `pending` byte per actor.
// Only an actor's own lane, or its bucket's block while it forms the inbox, writes its two bytes; k_listing_plan
// (after the apply) reads the counts and writes `due`, `changed` and `seen`.
constexpr uint32_t kRcListPtr = 6;
constexpr uint32_t kLsMail = 4, kLsChanged = 5, kLsPend = 6, kLsPlanned = 7, kLsCtr = 8, kLsLast = 16, kLsPayload = 24,
                   kLsSeen = 32, kLsDueOff = 48;
constexpr uint32_t kLsSubscribes = 0, kLsFinds = 1, kLsSent = 2, kLsNotified = 3;
__host__ __device__ __forceinline__ size_t ls_cnt_off(uint32_t nb) { return ((size_t)kLsDueOff + nb + 3u) & ~(size_t)3; }
__host__ __device__ __forceinline__ size_t ls_mask_off(uint32_t nk, uint32_t nb) { return ls_cnt_off(nb) + 2ull * nk * nb; }
__host__ __device__ __forceinline__ size_t ls_words(uint32_t nk, uint32_t nb, uint32_t bb) {
  return ((ls_mask_off(nk, nb) + 3u) & ~(size_t)3) + 2ull * (((size_t)nb << bb) / 4u);
}
struct ListDev {
  uint32_t* base;
  uint8_t *sub, *pend;  // [nb << bb] each
  uint32_t nk, nb;
  __device__ __forceinline__ uint32_t* due(uint32_t b) const { return base + kLsDueOff + b; }
  __device__ __forceinline__ uint32_t* cnt_u(uint32_t k, uint32_t b) const { return base + ls_cnt_off(nb) + (size_t)k * nb + b; }
  __device__ __forceinline__ uint32_t* cnt_p(uint32_t k, uint32_t b) const {
    return base + ls_cnt_off(nb) + (size_t)(nk + k) * nb + b;
  }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kLsCtr) + i;
  }
  __device__ __forceinline__ unsigned long long* last(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kLsLast) + i;
  }
  __device__ __forceinline__ unsigned long long* seen(uint32_t k) const {
    return reinterpret_cast<unsigned long long*>(base + kLsSeen) + k;
  }
};
__device__ __forceinline__ ListDev list_dev(uint32_t* base) {
  ListDev d;
  d.base = base;
  d.nk = base[0];
  d.nb = base[1];
  d.sub = reinterpret_cast<uint8_t*>(base + ((ls_mask_off(d.nk, d.nb) + 3u) & ~(size_t)3));
  d.pend = d.sub + ((size_t)d.nb << base[2]);
  return d;
}
__device__ __forceinline__ ListDev list_dev_of(const uint32_t* recep) {
  return list_dev(*reinterpret_cast<uint32_t* const*>(recep + kRcListPtr));
}
// the same for a caller that knows the shape (the receptionist's n_keys and nb, the launch's bb): the address is the
// only load, beside the receptionist's own header and not after it
__device__ __forceinline__ uint32_t* list_base_of(const uint32_t* recep) {
  return *reinterpret_cast<uint32_t* const*>(recep + kRcListPtr);
}
__device__ __forceinline__ ListDev list_dev_with(const uint32_t* recep, uint32_t nk, uint32_t nb, uint32_t bb) {
  ListDev d;
  d.base = list_base_of(recep);
  d.nk = nk;
  d.nb = nb;
  d.sub = reinterpret_cast<uint8_t*>(d.base + ((ls_mask_off(nk, nb) + 3u) & ~(size_t)3));
  d.pend = d.sub + ((size_t)nb << bb);
  return d;
}
// what one thread's drains did: counted in registers, added to the storage once per wave (listing_commit)
struct ListCount {
  uint32_t sub, find, chg, pend;  // chg: a mask byte was stored; pend: a pending bit was set
};

// compiled_apply of the listings instantiations: compiled_apply_tp plus AGX_A_SUBSCRIBE_LISTING / AGX_A_FIND against
// the actor's two mask bytes `sb` / `pd` (registers of the drain); neither touches the emitter.  A function of its
// own: every other instantiation compiles compiled_apply_tp / compiled_apply_rc as before.
// (The third copy of those cases: a fix here belongs in compiled_apply_rc and compiled_apply_tp too.)
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_ls(const DevParams& P, const RecepDev& RD, const TopicDev& TP, uint32_t& kind,
                                                      uint32_t self, uint64_t* w, uint32_t src, uint32_t pay, uint32_t& mk,
                                                      RecepCount& rc, uint32_t q, uint32_t& npub, uint32_t& sb, uint32_t& pd,
                                                      ListCount& lc, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, rc_operand(RD, C.src1, C.word1, C.k1, pay, w, src, self),
                rc_operand(RD, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, rc_operand(RD, C.src3, C.word3, C.k3, pay, w, src, self),
                rc_operand(RD, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = rc_operand(RD, A.src, A.sword, A.k, pay, w, src, self);
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      const uint32_t bit = 1u << (A.pad1 & 7u);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_REGISTER:
          if (!(mk & bit)) {
            mk |= bit;
            ++rc.reg;
          }
          break;
        case AGX_A_DEREGISTER:
          if (mk & bit) {
            mk &= ~bit;
            ++rc.dereg;
          }
          break;
        case AGX_A_PUBLISH: {
          const uint32_t slot = atomicAdd(TP.base + kTpCursor, 1u);
          if (slot < TP.cap) TP.stage()[slot] = make_uint4(self, q, A.pad1 & 7u, msg);
          ++npub;
          break;
        }
        case AGX_A_SUBSCRIBE_LISTING:  // Subscribe(key, self): the immediate reply is owed on every Subscribe
          sb |= bit;
          pd |= bit;
          ++lc.sub;
          break;
        case AGX_A_FIND:  // Find(key, self)
          pd |= bit;
          ++lc.find;
          break;
        case AGX_A_TELL:
        case AGX_A_ROUTE: {
          uint64_t d = 0;
          if (A.op == AGX_A_TELL || (A.pad0 & AGX_ROUTE_BY_INDEX)) {
            if (A.dsrc == AGX_V_SELF && A.op == AGX_A_TELL) {  // (self + dk) mod n: ring neighbours
              int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
              d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
            } else {
              d = rc_operand(RD, A.dsrc, A.dword, A.dk, pay, w, src, self);
            }
          }
          uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
          if (A.op == AGX_A_ROUTE) {
            const uint32_t key = A.pad1 & 7u;
            if (A.pad0 & AGX_ROUTE_BY_INDEX) {
              ref = RD.at(key, d);
            } else {
              ref = RD.successor(key, w[A.word & 1u]);
              if (ref != kRcNone) w[A.word & 1u] = (uint64_t)ref + 1ull;  // (no routee: the cursor stays)
            }
            if (ref == kRcNone) ++rc.none;
            else ++rc.routed;
          }
          if (A.pad0 & AGX_ROUTE_KEEP_SENDER) {  // a forward: the envelope keeps the incoming message's sender
            const uint32_t me = emit.self;
            emit.self = src;
            emit(ref, msg);
            emit.self = me;
          } else {
            emit(ref, msg);
          }
          break;
        }
        default: break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// ---- consistent-hashing and random routing (agx_set_router_logics; TY/internal/routing/
// RoutingLogic.scala:77-112, akka-actor routing/ConsistentHash.scala:25-139, routing/MurmurHash.scala:37-129), on top of
// the receptionist.  An allocation of its own whose address stands in words [kRcHashPtr, kRcHashPtr + 2) of the
// receptionist's storage, u32 units:
//   [0] hashed_keys_mask   [1] virtual_nodes_factor   [2] npts: the ring points of all actors (n_actors x factor; 0
//       with an empty mask)   [3] nseg: segments of kHrSeg points   [4..5] the seed of random routing (u64)
//   [8..13]  three u64 counters: hashed, random, ring_rebuilds   [16..23] ring_size[k] of the ring in force
//   [kHrSegOff + slot * nseg + s]  segcnt: the members of the key in segment s of the static ring (k_hash_count), then
//   segoff[slot * nseg + s]: their offset in the key's ring (k_hash_scan); slot = the key's rank among the hashed keys
//   then the static ring, npts hashes and npts ids sorted by (signed hash, id): every actor's points, built once
//   then per slot the key's ring, npts hashes and npts ids: the stable compaction of the static ring by the key's
//   mask bit (k_hash_fill), rewritten between two applies only
// The drains only read the rings in force and the header.
constexpr uint32_t kRcHashPtr = 20;
constexpr uint32_t kHrMask = 0, kHrFactor = 1, kHrNpts = 2, kHrNseg = 3, kHrSeed = 4, kHrCtr = 8, kHrSize = 16, kHrSegOff = 32;
constexpr uint32_t kHrHashed = 0, kHrRandom = 1, kHrRebuilds = 2;
constexpr uint32_t kHrSeg = 1024;
constexpr uint32_t kHrRandomTag = 0x02000000u;  // fanout_rand's domain of random routing (0: fan-out, 0x04.., 0x08..: gossip)
__host__ __device__ __forceinline__ size_t hr_static_off(uint32_t nslots, uint32_t nseg) {
  return (size_t)kHrSegOff + 2ull * nslots * nseg;
}
__host__ __device__ __forceinline__ size_t hr_words(uint32_t nslots, uint32_t nseg, uint32_t npts) {
  return hr_static_off(nslots, nseg) + 2ull * npts * (1ull + nslots);
}
struct HashDev {
  uint32_t* base;
  uint32_t hmask, npts, nseg, nslots;
  __device__ __forceinline__ uint32_t slot(uint32_t k) const { return (uint32_t)__popc(hmask & ((1u << k) - 1u)); }
  __device__ __forceinline__ uint32_t* segcnt(uint32_t sl) const { return base + kHrSegOff + (size_t)sl * nseg; }
  __device__ __forceinline__ uint32_t* segoff(uint32_t sl) const { return base + kHrSegOff + (size_t)(nslots + sl) * nseg; }
  __device__ __forceinline__ uint32_t* st_hash() const { return base + hr_static_off(nslots, nseg); }
  __device__ __forceinline__ uint32_t* st_id() const { return st_hash() + npts; }
  __device__ __forceinline__ uint32_t* ring_hash(uint32_t sl) const { return st_hash() + 2ull * npts * (1ull + sl); }
  __device__ __forceinline__ uint32_t* ring_id(uint32_t sl) const { return ring_hash(sl) + npts; }
  __device__ __forceinline__ unsigned long long* ctr(uint32_t i) const {
    return reinterpret_cast<unsigned long long*>(base + kHrCtr) + i;
  }
};
__device__ __forceinline__ HashDev hash_dev(uint32_t* base) {
  HashDev h;
  h.base = base;
  h.hmask = base[kHrMask];
  h.npts = base[kHrNpts];
  h.nseg = base[kHrNseg];
  h.nslots = (uint32_t)__popc(h.hmask);
  return h;
}
__device__ __forceinline__ uint32_t* hash_base_of(const uint32_t* recep) {
  return *reinterpret_cast<uint32_t* const*>(recep + kRcHashPtr);
}

// MurmurHash.scala:37-100 in wrapping 32-bit arithmetic (Java Int: `>>>` is the unsigned shift)
__host__ __device__ __forceinline__ uint32_t mm_extend(uint32_t h, uint32_t v, uint32_t ma, uint32_t mb) {
  const uint32_t x = v * ma;
  return (h ^ (((x << 11) | (x >> 21)) * mb)) * 3u + 0x52dce729u;
}
__host__ __device__ __forceinline__ uint32_t mm_finalize(uint32_t h) {
  uint32_t i = h ^ (h >> 16);
  i *= 0x85ebca6bu;
  i ^= i >> 13;
  i *= 0xc2b2ae35u;
  i ^= i >> 16;
  return i;
}
// MurmurHash.stringHash (MurmurHash.scala:115-129) of x as an unsigned decimal string without padding: the digits as
// ten BCD nibbles (divisions by constants), two characters per extendHash step, an odd last one alone
__host__ __device__ __forceinline__ uint32_t mm_decimal_hash(uint32_t x) {
  uint64_t bcd = 0;
  uint32_t len = 1, r = x;
#pragma unroll
  for (uint32_t i = 0; i < 10; ++i) {
    const uint32_t q = r / 10u, d = r - q * 10u;
    bcd |= (uint64_t)d << (4u * i);
    len = d ? i + 1u : len;
    r = q;
  }
  uint32_t h = (len * 0xf7ca7fd2u) ^ 0x971e137bu, c = 0x95543787u, k = 0x2ad7eb25u, j = 0;
  for (; j + 1u < len; j += 2u) {  // (character j is nibble len - 1 - j)
    const uint32_t c0 = 0x30u + (uint32_t)((bcd >> (4u * (len - 1u - j))) & 15u);
    const uint32_t c1 = 0x30u + (uint32_t)((bcd >> (4u * (len - 2u - j))) & 15u);
    h = mm_extend(h, (c0 << 16) + c1, c, k);
    c = c * 5u + 0x7b7d159cu;
    k = k * 5u + 0x6bce6396u;
  }
  if (j < len) h = mm_extend(h, 0x30u + (uint32_t)(bcd & 15u), c, k);
  return mm_finalize(h);
}
// ConsistentHash.concatenateNodeHash (ConsistentHash.scala:134-139)
__host__ __device__ __forceinline__ uint32_t mm_node_point(uint32_t node_hash, uint32_t vnode) {
  return mm_finalize(mm_extend(node_hash ^ 0x971e137bu, vnode, 0x95543787u, 0x2ad7eb25u));
}
// ConsistentHash.nodeFor(x.toString) (ConsistentHash.scala:76-83,100-110) on the ring of n points: the id of the first
// entry with hash >= stringHash(str(x)) as signed integers, else of entry 0 (none: an empty ring).  Inlined: kept out
// of line the two instantiations spill more (81 / 64 VGPRs against 62 / 62: the call keeps the drain's registers live
// across it).
__device__ __forceinline__ uint32_t hr_node_for(const uint32_t* rh, const uint32_t* rid, uint32_t n, uint32_t x) {
  if (!n) return kRcNone;
  const int32_t h = (int32_t)mm_decimal_hash(x);
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((int32_t)rh[mid] < h) lo = mid + 1u;
    else hi = mid;
  }
  return rid[lo == n ? 0u : lo];
}
// what one thread's drains routed by the two logics: added to the counters once per wave (hash_commit)
struct HashCount {
  uint32_t hashed, random;
};

// compiled_apply of the router-logics instantiations: compiled_apply_rc plus AGX_ROUTE_HASHED and AGX_ROUTE_RANDOM on
// AGX_A_ROUTE.  A function of its own: every other instantiation compiles compiled_apply_rc as before.  (Its other
// cases are compiled_apply_rc's: a fix to one of them belongs in both.)
template <typename Emit>
__device__ __forceinline__ uint32_t compiled_apply_hr(const DevParams& P, const RecepDev& RD, const HashDev& HD, uint32_t& kind,
                                                      uint32_t self, uint64_t* w, uint32_t src, uint32_t pay, uint32_t& mk,
                                                      RecepCount& rc, HashCount& hc, Emit& emit) {
  const uint32_t b = kind - AGX_KIND_COMPILED;
  if (b >= P.n_beh) return AGX_RES_UNHANDLED;
  const uint32_t c1 = P.bfirst[b + 1];
  for (uint32_t c = P.bfirst[b]; c < c1; ++c) {
    const agx_case C = P.bcase[c];
    if (!cb_cmp(C.cmp1, rc_operand(RD, C.src1, C.word1, C.k1, pay, w, src, self),
                rc_operand(RD, C.src2, C.word2, C.k2, pay, w, src, self)))
      continue;
    if (!cb_cmp(C.cmp2, rc_operand(RD, C.src3, C.word3, C.k3, pay, w, src, self),
                rc_operand(RD, C.src4, C.word4, C.k4, pay, w, src, self)))
      continue;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      const agx_act A = P.bact[i];
      const uint64_t v = rc_operand(RD, A.src, A.sword, A.k, pay, w, src, self);
      const uint32_t msg = A.or_mask ? ((uint32_t)v & 0xFFFFFFu) | A.or_mask : (uint32_t)v;
      const uint32_t bit = 1u << (A.pad1 & 7u);
      switch (A.op) {
        case AGX_A_SET: w[A.word & 1u] = v; break;
        case AGX_A_ADD: w[A.word & 1u] += v; break;
        case AGX_A_MAX: w[A.word & 1u] = v > w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_MIN: w[A.word & 1u] = v < w[A.word & 1u] ? v : w[A.word & 1u]; break;
        case AGX_A_REGISTER:
          if (!(mk & bit)) {
            mk |= bit;
            ++rc.reg;
          }
          break;
        case AGX_A_DEREGISTER:
          if (mk & bit) {
            mk &= ~bit;
            ++rc.dereg;
          }
          break;
        case AGX_A_TELL:
        case AGX_A_ROUTE: {
          uint64_t d = 0;
          if (A.op == AGX_A_TELL || (A.pad0 & (AGX_ROUTE_BY_INDEX | AGX_ROUTE_HASHED))) {
            if (A.dsrc == AGX_V_SELF && A.op == AGX_A_TELL) {  // (self + dk) mod n: ring neighbours
              int64_t x = ((int64_t)self + A.dk) % (int64_t)P.n_global;
              d = (uint64_t)(x < 0 ? x + (int64_t)P.n_global : x);
            } else {
              d = rc_operand(RD, A.dsrc, A.dword, A.dk, pay, w, src, self);
            }
          }
          uint32_t ref = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
          if (A.op == AGX_A_ROUTE) {
            const uint32_t key = A.pad1 & 7u;
            if (A.pad0 & AGX_ROUTE_HASHED) {  // (a key outside the mask was refused at agx_run)
              const uint32_t sl = HD.slot(key);
              ref = ((HD.hmask >> key) & 1u) ? hr_node_for(HD.ring_hash(sl), HD.ring_id(sl), HD.base[kHrSize + key], (uint32_t)d)
                                             : kRcNone;
              if (ref != kRcNone) ++hc.hashed;
            } else if (A.pad0 & AGX_ROUTE_RANDOM) {
              const uint32_t n = RD.size(key);
              if (n) {  // (no routee: the counter stays)
                const uint64_t seed = *reinterpret_cast<const uint64_t*>(HD.base + kHrSeed);
                const uint32_t cn = (uint32_t)w[A.word & 1u];
                ref = RD.list(key)[(uint32_t)(fanout_rand(seed, self, (cn & 0x00FFFFFFu) | kHrRandomTag, 0) % n)];
                w[A.word & 1u] += 1ull;
                ++hc.random;
              } else {
                ref = kRcNone;
              }
            } else if (A.pad0 & AGX_ROUTE_BY_INDEX) {
              ref = RD.at(key, d);
            } else {
              ref = RD.successor(key, w[A.word & 1u]);
              if (ref != kRcNone) w[A.word & 1u] = (uint64_t)ref + 1ull;  // (no routee: the cursor stays)
            }
            if (ref == kRcNone) ++rc.none;
            else ++rc.routed;
          }
          if (A.pad0 & AGX_ROUTE_KEEP_SENDER) {  // a forward: the envelope keeps the incoming message's sender
            const uint32_t me = emit.self;
            emit.self = src;
            emit(ref, msg);
            emit.self = me;
          } else {
            emit(ref, msg);
          }
          break;
        }
        default: break;
      }
    }
    if (C.result == AGX_RES_BECOME) {
      kind = AGX_KIND_COMPILED + C.next;
      return AGX_RES_SAME;
    }
    return C.result;
  }
  return AGX_RES_UNHANDLED;
}

// Can a behaviour of the kind mask KM read its message's sender (`src` of apply_msg below)?  False
// only for masks all of whose kinds provably ignore it there: RING (its case uses w, pay and self).
// Compiled behaviours (an operand may be the sender), PingPong (replies to it), the CRDT kinds and
// every mixed mask stay true.  A launch specialised to a sender-free mask need not load the inbox's
// sender array (k_dense_fused / k_dense_apply); the tells it WRITES still carry their sender.
constexpr bool km_reads_sender(uint32_t KM) { return KM != kb(AGX_KIND_RING); }

// `kind` is the actor's current behaviour: a compiled behaviour's become updates it (the caller
// keeps it for the rest of the drain and stores it back).
template <uint32_t KM, typename Emit>
__device__ __forceinline__ uint32_t apply_msg(const DevParams& P, uint32_t& kind_io, uint32_t self, uint32_t local,
                                              uint64_t* w, uint32_t src, uint32_t pay, Emit&& emit, uint32_t nstash = 0) {
  constexpr bool kStash = (KM & kStashKM) != 0;
  uint32_t kind = kind_io;
  if constexpr (KM == kb(AGX_KIND_RING)) kind = AGX_KIND_RING;  // single-kind specialisations: no dispatch
  if constexpr (KM == kb(AGX_KIND_FORWARD_RR)) kind = AGX_KIND_FORWARD_RR;
  if constexpr (KM == kb(AGX_KIND_FANOUT)) kind = AGX_KIND_FANOUT;
  if constexpr (KM == kb(AGX_KIND_COUNTER)) kind = AGX_KIND_COUNTER;
  if constexpr ((KM & kb(AGX_KIND_COMPILED)) != 0)
    if (kind >= AGX_KIND_COMPILED) return compiled_apply<kStash>(P, kind_io, self, w, src, pay, emit, nstash);
  switch (kind) {
    case AGX_KIND_COUNTER:
      if constexpr ((KM & kb(AGX_KIND_COUNTER)) != 0) {
        w[0] += 1;
        w[1] += pay;  // w[1] exists (array of AGX_MAX_WORDS); only stored back if W > 1
      }
      return AGX_RES_SAME;
    case AGX_KIND_RING:
      if constexpr ((KM & kb(AGX_KIND_RING)) != 0) {
        w[0] += 1;
        if (pay > 0) {
          uint32_t d = self + P.ring_stride;  // both < n_global < 2^31: no overflow, one conditional subtract
          emit(d >= P.n_global ? d - P.n_global : d, pay - 1);
        }
      }
      return AGX_RES_SAME;
    case AGX_KIND_FANOUT:
      if constexpr ((KM & kb(AGX_KIND_FANOUT)) != 0) {
        w[0] += 1;
        w[1] += pay;
        const uint32_t ttl = pay >> 24, h = pay & 0x00FFFFFFu;  // ttl 8 bits, hash 24 bits
        if (ttl > 0)
          for (uint32_t j = 0; j < P.fan_k; ++j) {
            uint64_t r = fanout_rand(P.fan_seed, self, h, j);
            uint32_t d = zipf_dest(P.zipf_cdf, P.zipf_perm, P.zipf_ent, r);
            emit(d, ((ttl - 1) << 24) | ((uint32_t)r & 0x00FFFFFFu));
          }
      }
      return AGX_RES_SAME;
    case AGX_KIND_FORWARD_RR:
      if constexpr ((KM & kb(AGX_KIND_FORWARD_RR)) != 0) {
        w[0] += 1;
        if (pay > 0) {
          uint64_t b = P.row_ptr[local], deg = P.row_ptr[local + 1] - b;
          if (deg) {
            // cursor mod degree; 32-bit remainder when both fit (the common case)
            uint64_t r = (w[1] <= 0xFFFFFFFFull && deg <= 0xFFFFFFFFull) ? (uint64_t)((uint32_t)w[1] % (uint32_t)deg)
                                                                         : w[1] % deg;
            uint64_t e = b + r;
            w[1] += 1;
            emit(P.col[e], pay - 1);
          }
        }
      }
      return AGX_RES_SAME;
    case AGX_KIND_STOP_AFTER:
      if constexpr ((KM & kb(AGX_KIND_STOP_AFTER)) != 0) {
        w[0] += 1;
        return (w[0] >= w[1]) ? AGX_RES_STOPPED : AGX_RES_SAME;
      }
      return AGX_RES_SAME;
    case AGX_KIND_PINGPONG:
      if constexpr ((KM & kb(AGX_KIND_PINGPONG)) != 0) {
        // BenchmarkActors.PingPong (akka-bench-jmh/.../actor/BenchmarkActors.scala:20-32)
        uint32_t res = (w[0] == 0) ? AGX_RES_STOPPED : AGX_RES_SAME;
        w[1] += 1;
        emit(src, pay);
        w[0] -= 1;
        return res;
      }
      return AGX_RES_SAME;
    case AGX_KIND_EVEN:
      if constexpr ((KM & kb(AGX_KIND_EVEN)) != 0) {
        if (pay & 1u) return AGX_RES_UNHANDLED;
        w[0] += 1;
      }
      return AGX_RES_SAME;
    default:
      return AGX_RES_SAME;
  }
}

}  // namespace agx
