// agx_lwwmap_delta.h — delta replication of LWWMap replicas on the device (include/akka_gpu.h
// "LWWMap delta replication"; agx_set_lwwmap_delta):
//
//   ORMap.DeltaOp (PutDeltaOp, RemoveDeltaOp, DeltaGroup.merge)   DD/ORMap.scala:30-164
//   ORMap.put / remove (the deltas they record)                   DD/ORMap.scala:254-265,361-366
//   ORMap.dryMergeDelta / mergeDelta                              DD/ORMap.scala:425-503
//   ORSet.AddDeltaOp.merge, add / remove deltas                   DD/ORSet.scala:57-76,339-351,380-387
//   ORSet.mergeDelta / mergeRemoveDelta                           DD/ORSet.scala:455-501
//   DeltaPropagationSelector, receiveDeltaPropagation             as agx_crdt.h
//
// Variant V_LWWMAP_DELTA follows V_LWWMAP's split.  lwd_protocol (one lane per replica, inside
// k_bucket_apply) does the tells, the row allocation in message order, the void slots of the
// NoDeltaPlaceholder groups and the unhandled count: it only READS the replica (deltaCounter, round
// robin, deltaSentToNode, the ring's {type, key} words) and simulates the selector over the run.
// k_lwwmap_delta_merge (one wave per replica, lane k = key k AND ring slot k) then applies the run's
// state effects and writes every word of the replica that changes: data, envelope, selector and ring.
#pragma once
#include "agx_lwwmap.h"

namespace agx {

constexpr uint32_t kLdEnv = 2u * AGX_LWWMAP_WORDS;                 // u32 index of deltaVersions[8]
constexpr uint32_t kLdRing = kLdEnv + 2u * AGX_DELTA_ENV_WORDS;    // u32 index of the ring
constexpr uint32_t kLdEnt = AGX_LWWMAP_DELTA_LOG_U32;              // u32 per ring entry
constexpr uint32_t kLdPutRec = 5u, kLdRemRec = 9u;                 // u32 per op record of a DeltaPropagation row
static_assert(kLdEnv == 712u && kLdRing == 736u && kLdEnv % 4u == 0 && kLdRing % 16u == 0,
              "LWWMap delta state: 712 data u32, 24 envelope u32, then the ring, every entry 64-B aligned");
static_assert(kLdRing + AGX_DELTA_LOG * kLdEnt == 2u * AGX_LWWMAP_DELTA_WORDS && AGX_LWWMAP_DELTA_WORDS == 880u &&
                  AGX_LWWMAP_DELTA_WORDS <= AGX_MAX_GENERAL_WORDS && AGX_LWWMAP_DELTA_WORDS % 16u == 0,
              "LWWMap delta state: 356 + 12 + 512 = 880 u64, whole 128-B lines");
static_assert(AGX_DELTA_LOG == kWave, "one lane per ring slot");
// a group has fewer than max-delta-size ops (a single seqNr: one op), the widest op is a remove
static_assert(12u + kLdRemRec * (AGX_DELTA_MAX_SIZE - 1u) == AGX_LWWMAP_DELTA_ROW_U32, "the widest DeltaPropagation row");
static_assert(kLwRowMax + AGX_CRDT_NODES == AGX_LWWMAP_DELTA_STATE_ROW_U32, "the widest full-state row with deltaVersions");
constexpr uint32_t kLdPitch = (AGX_LWWMAP_DELTA_STATE_ROW_U32 + 31u) / 32u * 32u;  // (enable_lwwmap_delta: the engine's row pitch)
static_assert(kLdPitch == 768u && AGX_LWWMAP_DELTA_ROW_U32 < kLdPitch - 1u && AGX_LWWMAP_DELTA_STATE_ROW_U32 < kLdPitch - 1u,
              "both row forms fit the row pitch, below the length word of a DeltaPropagation (pitch - 1)");

constexpr uint32_t kLdProp = 5, kLdTick = 6;  // (after kLwMerge, kLwPut, kLwRemove, kLwSnap)
__device__ __forceinline__ uint32_t lwd_code(uint32_t sv, uint32_t pv) {
  if (is_wide(sv)) return (pv >> 30) != kLwType ? 0u : (pv & AGX_DELTA_ROW_BIT) ? kLdProp : kLwMerge;
  const uint32_t op = pv >> 24, arg = pv & 0xFFFFFFu;
  if (op == AGX_OP_PUT) return kLwPut;
  if (op == AGX_OP_REMOVE) return arg < AGX_ORSET_ELEMS ? kLwRemove : 0u;
  if (op == AGX_OP_GOSSIP) return kLwSnap;
  if (op == AGX_OP_DELTA_TICK) return kLdTick;
  return 0u;
}
// the ring's {type, key} word of a local update
__device__ __forceinline__ uint32_t lwd_tk(uint32_t c, uint32_t arg) {
  return (c == kLwPut ? 1u : 2u) | ((arg & (AGX_ORSET_ELEMS - 1u)) << 8);
}
// the writer client's seeded update of DELTA_TICK countdown k (include/akka_gpu.h)
__device__ __forceinline__ uint32_t lwd_writer_op(const DevParams& P, uint32_t self, uint32_t k) {
  const uint64_t r = fanout_rand(P.gossip_seed, self, k | 0x04000000u, 0);
  const uint32_t key = (uint32_t)(r >> 48) & 7u;
  return ((r >> 40) & 3u) ? AGX_OP(AGX_OP_PUT, AGX_OP_PUT_ARG(key, (uint32_t)(r >> 8) & AGX_LWWMAP_VALUE_MAX)) : AGX_OP(AGX_OP_REMOVE, key);
}
__device__ __forceinline__ const uint32_t* lwd_state32(const DevParams& P, uint32_t l) {
  return reinterpret_cast<const uint32_t*>(wide_state(P, l));  // (actor-major: prepare_run)
}
__device__ __forceinline__ void lwd_sim_load(const DevParams& P, uint32_t l, DeltaSim& ds) {
  const uint32_t* su = lwd_state32(P, l);
  ds.on = true;
  ds.ctr = su[kLdEnv + 8];
  ds.rr = su[kLdEnv + 9];
#pragma unroll
  for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) ds.sent[n] = su[kLdEnv + 10 + n];
}

// phase A (per lane): the tells one message will produce (a NoDeltaPlaceholder group's void slot included,
// as crdt_count counts it); *rows += its rows
__device__ __forceinline__ uint32_t lwd_count(const DevParams& P, uint32_t self, uint32_t l, uint32_t src, uint32_t pay,
                                              uint32_t* rows, DeltaSim& ds) {
  const uint32_t c = lwd_code(src, pay);
  const uint32_t arg = pay & 0xFFFFFFu;
  if (c == kLwSnap) {
    const uint32_t f = P.n_global > 1 && key_size(self, P.n_global) > 1 ? P.gossip_f : 0u;
    *rows += f ? 1u : 0u;
    return f + (arg > 0 ? 1u : 0u);
  }
  if (c != kLwPut && c != kLwRemove && c != kLdTick) return 0;
  if (!ds.on) lwd_sim_load(P, l, ds);
  if (c != kLdTick) {
    ++ds.ctr;
    return 0;
  }
  uint32_t t = (arg & AGX_DELTA_WRITE) ? 1u : 0u;
  const uint32_t node = self % AGX_CRDT_NODES, na = key_size(self, P.n_global) - 1u;
  if (na) {
    const uint32_t sz = dl_slice_size(na);
    const uint32_t s = na <= sz ? na : sz;
    for (uint32_t i = 0; i < s; ++i) {
      const uint32_t x = dl_slice_node(node, na, sz, ds.rr, i);
      uint32_t sx = 0;
#pragma unroll
      for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) sx = n == x ? ds.sent[n] : sx;
      if (ds.ctr > sx) {
        ++t;
        ++*rows;
#pragma unroll
        for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) ds.sent[n] = n == x ? ds.ctr : ds.sent[n];
      }
    }
    ds.rr += sz;
  }
  return t + ((arg & 0xFFFFu) > 0 ? 1u : 0u);
}

// Is the group of seqNrs (j, ctr] a NoDeltaPlaceholder?  collectPropagations reduces the entries from the left
// and checks deltaSize after every merge, so a single entry never is one; deltaSize only grows, so the group is
// one iff its final number of ops reaches max-delta-size.  A put coalesces iff the entry before it is a put of
// the same key (the group's last op then is that put, coalesced or not).  Only {type, key} words decide: those
// of seqNrs <= ctr0 from the ring as the run found it, the later ones from the run's own messages.
template <typename Src, typename Pay>
__device__ __forceinline__ bool lwd_group_ph(const DevParams& P, const uint32_t* su, uint32_t ctr0, uint32_t j, uint32_t ctr,
                                             uint32_t s0, uint32_t nd, const Src& isrc, const Pay& ipay) {
  const uint32_t cnt = ctr - j;
  if (cnt < 2u) return false;
  if (P.delta_max <= 1u || cnt > AGX_DELTA_LOG) return true;  // (more than the ring holds: AGX_ECAPACITY was raised)
  uint32_t nops = 0, prev = 0, own = 0, mq = 0;
  for (uint32_t q = j + 1u; q <= ctr; ++q) {
    uint32_t tk = 0;
    if (q <= ctr0) {
      tk = su[kLdRing + kLdEnt * (q % AGX_DELTA_LOG) + 1u];
    } else {  // the (q - ctr0)-th recording message of the run (the walk resumes where it stopped)
      while (mq < nd) {
        const uint32_t sv = isrc(s0 + mq), pv = ipay(s0 + mq);
        ++mq;
        const uint32_t c = lwd_code(sv, pv);
        if (c == kLwPut || c == kLwRemove) {
          ++own;
          tk = lwd_tk(c, pv & 0xFFFFFFu);
          if (own == q - ctr0) break;
        }
      }
    }
    nops += ((tk & 0xFFu) == 1u && tk == prev) ? 0u : 1u;
    prev = tk;
  }
  return nops >= P.delta_max;
}

// phase B (per lane): tells, row handles and void slots in message order; returns the unhandled count;
// *state_work: the run reads or writes the state (k_lwwmap_delta_merge then walks it)
template <typename Emit, typename Src, typename Pay>
__device__ __forceinline__ uint32_t lwd_protocol(const DevParams& P, uint32_t self, uint32_t l, uint32_t s0, uint32_t nd,
                                                 const Src& isrc, const Pay& ipay, uint32_t& row_cursor, Emit& em,
                                                 bool* state_work) {
  const uint32_t m = key_size(self, P.n_global), node = self % AGX_CRDT_NODES, na = m - 1u;
  const uint32_t f = P.n_global > 1 && m > 1 ? P.gossip_f : 0u;
  const uint32_t* su = lwd_state32(P, l);
  DeltaSim ds;
  ds.on = false;
  uint32_t ctr0 = 0, nunh = 0, nmod = 0;
  const uint32_t rc0 = row_cursor;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(s0 + q), pv = ipay(s0 + q);
    const uint32_t c = lwd_code(sv, pv);
    const uint32_t arg = pv & 0xFFFFFFu;
    if (c == 0) {
      ++nunh;
      continue;
    }
    if (c == kLwSnap) {
      if (f) {
        const uint32_t tagged = (kLwType << 30) | row_cursor++;
        for (uint32_t i = 0; i < f; ++i) em.wide(crdt_key_peer(P.gossip_seed, self, arg, i, P.n_global), tagged);
      }
      if (arg > 0) em(self, AGX_OP(AGX_OP_GOSSIP, arg - 1u));
      continue;
    }
    ++nmod;
    if (c == kLwMerge || c == kLdProp) continue;
    if (!ds.on) {
      lwd_sim_load(P, l, ds);
      ctr0 = ds.ctr;
    }
    if (c != kLdTick) {
      ++ds.ctr;
      continue;
    }
    const uint32_t k = arg & 0xFFFFu;
    if (arg & AGX_DELTA_WRITE) em(self, lwd_writer_op(P, self, k));
    if (na) {
      const uint32_t sz = dl_slice_size(na), cnt = na <= sz ? na : sz;
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t x = dl_slice_node(node, na, sz, ds.rr, i);
        uint32_t j = 0;
#pragma unroll
        for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) j = n == x ? ds.sent[n] : j;
        if (ds.ctr <= j) continue;  // deltaEntriesAfter(j) is empty
        const uint32_t h = row_cursor++;
#pragma unroll
        for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) ds.sent[n] = n == x ? ds.ctr : ds.sent[n];
        if (lwd_group_ph(P, su, ctr0, j, ds.ctr, s0, q, isrc, ipay)) em.void_slot();
        else em.wide(self - node + x, (kLwType << 30) | AGX_DELTA_ROW_BIT | h);
      }
      ds.rr += sz;
    }
    if (k > 0) em(self, AGX_OP(AGX_OP_DELTA_TICK, (k - 1u) | (arg & AGX_DELTA_WRITE)));
  }
  *state_work = nmod != 0 || row_cursor != rc0;
  return nunh;
}

__device__ __forceinline__ uint64_t lwd_rotr(uint64_t x, uint32_t r) {
  r &= 63u;
  return r ? (x >> r) | (x << (64u - r)) : x;
}
__device__ __forceinline__ uint32_t lwd_pick(const uint32_t (&a)[AGX_CRDT_NODES], uint32_t x) {
  uint32_t v = 0;
#pragma unroll
  for (uint32_t n = 0; n < AGX_CRDT_NODES; ++n) v = n == x ? a[n] : v;
  return v;
}

// One replica's run of nd messages (wave-uniform arguments, all 64 lanes converged).  Lane k holds key k's 8
// dots, timestamp and register word AND ring slot k's 16 u32; the wave holds the version vector, the
// deltaVersions and the selector words.  Every load of the replica's own state is issued before any
// dependent work; the messages are applied in order from registers; each piece is stored once at the end,
// only if changed.  Rows (snapshots and DeltaPropagation groups, in message order) from rc0 on.
template <typename Src, typename Pay>
__device__ __forceinline__ void lwwmap_delta_merge_wave(const DevParams& P, const CrdtHeap& H, uint32_t l, uint32_t node,
                                                        uint32_t nd, uint32_t rc0, uint32_t clock, int64_t now,
                                                        const Src& isrc, const Pay& ipay) {
  static_assert(AGX_ORSET_ELEMS == kWave, "one lane per LWWMap key");
  constexpr uint32_t vw = AGX_ORSET_ELEMS * AGX_CRDT_NODES / 2;  // first vvector word
  const uint32_t k = lane_id();
  const uint64_t lt = (1ull << k) - 1ull;  // the lanes below this one
  const uint32_t self = l;                 // (single rank)
  const uint32_t m = key_size(self, P.n_global), na = m - 1u;
  const uint32_t f = P.n_global > 1 && m > 1 ? P.gossip_f : 0u;
  uint64_t* st = wide_state(P, l);
  uint32_t* su = reinterpret_cast<uint32_t*>(st);
  uint4* se = reinterpret_cast<uint4*>(st + 4 * k);  // key k: 8 u32 dots = 2 x 16 B
  const uint4* sv4 = reinterpret_cast<const uint4*>(st + vw);
  int64_t* tp = reinterpret_cast<int64_t*>(st + AGX_LWWMAP_TS_WORD) + k;
  uint32_t* gp = su + AGX_LWWMAP_REG_U32 + k;
  uint4* ev4 = reinterpret_cast<uint4*>(su + kLdEnv);          // the envelope / selector area: 5 x 16 B used
  uint4* rg4 = reinterpret_cast<uint4*>(su + kLdRing + kLdEnt * k);  // ring slot k: 4 x 16 B
  const uint4 a0 = se[0], a1 = se[1], v0 = sv4[0], v1 = sv4[1];
  const uint4 x0 = ev4[0], x1 = ev4[1], x2 = ev4[2], x3 = ev4[3], x4 = ev4[4];
  const uint4 r0 = rg4[0], r1 = rg4[1], r2 = rg4[2], r3 = rg4[3];
  const int64_t ts0 = *tp;
  const uint32_t rg0 = *gp;
  uint32_t d[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  uint32_t cur[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  uint32_t dv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  uint32_t sent[8] = {x2.z, x2.w, x3.x, x3.y, x3.z, x3.w, x4.x, x4.y};
  uint32_t e[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
  uint32_t ctr = x2.x, rr = x2.y;
  int64_t ts = ts0;
  uint32_t rg = rg0;
  bool dirty = false, edirty = false;
  bool vch = false, dch = false, sch = false;  // the version vector / the deltaVersions / the selector words changed
  uint32_t h = rc0;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(q), pv = ipay(q);
    const uint32_t c = lwd_code(sv, pv);
    const uint32_t arg = pv & 0xFFFFFFu;
    if (c == kLwMerge) {  // a full-state gossip: as lwwmap_merge_wave, then DataEnvelope.merge of the deltaVersions behind the data
      const uint32_t* row = H.row(pv & kHandleMask);
      const uint32_t rm = reinterpret_cast<const uint8_t*>(row + kOrRowMask)[k];
      const uint32_t rc = __popc(rm);
      const uint32_t incl = wave_incl_sum(rc);
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
      uint32_t ro = kOrRowDots + incl - rc;
      const uint64_t lm = __ballot(rm != 0u);
      const uint32_t go = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm & lt);
      const uint32_t dvo = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm);  // (= the row's length word - 8)
      const uint4 va = *reinterpret_cast<const uint4*>(row + kOrRowVV), vb = *reinterpret_cast<const uint4*>(row + kOrRowVV + 4);
      uint32_t r[8], rdv[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) r[n] = (rm >> n) & 1u ? row[ro++] : 0u;
#pragma unroll
      for (int n = 0; n < 8; ++n) rdv[n] = row[dvo + n];
      const uint32_t rtl = rm ? row[go] : 0u, rth = rm ? row[go + 1] : 0u, rrg = rm ? row[go + 2] : 0u;
      const uint32_t rvv[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
      bool was = false, live = false;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        was |= d[n] != 0u;
        const uint32_t o = orset_merge_entry(d[n], r[n], cur[n], rvv[n]);
        dirty |= o != d[n];
        d[n] = o;
        live |= o != 0u;
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        vch |= rvv[n] > cur[n];
        dch |= rdv[n] > dv[n];
        cur[n] = max(cur[n], rvv[n]);
        dv[n] = max(dv[n], rdv[n]);
      }
      const int64_t rts = (int64_t)(((uint64_t)rth << 32) | rtl);
      const bool that = rm != 0u && (!was || rts > ts || (rts == ts && (rrg >> 24) < (rg >> 24)));
      ts = !live ? 0 : that ? rts : ts;
      rg = !live ? 0u : that ? rrg : rg;
    } else if (c == kLdProp) {  // receiveDeltaPropagation: causal delivery, then ORMap.mergeDelta
      const uint32_t* row = H.row(pv & kHandleMask);
      const uint32_t nops = row[0], from = row[1] % AGX_CRDT_NODES, lo = row[2], hi = row[3];
      const uint32_t seen = lwd_pick(dv, from);
      if ((nops & 0x80000000u) || seen >= hi || lo > seen + 1u) continue;  // a placeholder / handled / a seqNr is missing
      // dryMergeDelta over a copy: the copy's dots td, value (tval: present), version vector tvv
      uint32_t td[8], tvv[8];
      bool was = false;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        td[n] = d[n];
        tvv[n] = cur[n];
        was |= d[n] != 0u;
      }
      bool tval = was;
      int64_t tts = ts;
      uint32_t trg = rg;
      uint32_t o = 12;
      const uint32_t nmax = min(nops, AGX_DELTA_MAX_SIZE);
      for (uint32_t i = 0; i < nmax && o + kLdRemRec <= H.pw; ++i) {
        uint32_t x[kLdRemRec];  // the record at the width of the wider form, in one round trip (within the pitch: the loop's bound)
#pragma unroll
        for (uint32_t u = 0; u < kLdRemRec; ++u) x[u] = row[o + u];
        const uint32_t tk = x[0], key = (tk >> 8) & (AGX_ORSET_ELEMS - 1u);
        if ((tk & 0xFFu) == 1u) {  // PutDeltaOp: keys.mergeDelta(AddDeltaOp {key -> (from, ver)}, vvector (from, ver)); value overwritten
          const uint32_t ver = x[1], reg = x[2], tl = x[3], th = x[4];
          if (key == k) {
            bool here = false;
#pragma unroll
            for (int n = 0; n < 8; ++n) here |= td[n] != 0u;
#pragma unroll
            for (uint32_t n = 0; n < 8; ++n) {
              const uint32_t r = n == from ? ver : 0u;
              td[n] = here ? orset_merge_entry(td[n], r, tvv[n], r) : (r > tvv[n] ? r : 0u);
            }
            tval = true;
            tts = (int64_t)(((uint64_t)th << 32) | tl);
            trg = reg;
          }
#pragma unroll
          for (uint32_t n = 0; n < 8; ++n) tvv[n] = n == from ? max(tvv[n], ver) : tvv[n];
          o += kLdPutRec;
        } else {  // RemoveDeltaOp: the value dropped, mergeRemoveDelta (covered on every node, an unknown node has 0)
          uint32_t rvv[8];
#pragma unroll
          for (int n = 0; n < 8; ++n) rvv[n] = x[1 + n];
          if (key == k) {
            bool here = false, del = true;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
              here |= td[n] != 0u;
              del &= td[n] <= rvv[n];
            }
            if (here && del)
#pragma unroll
              for (int n = 0; n < 8; ++n) td[n] = 0u;
            tval = false;
            tts = 0;
            trg = 0u;
          }
#pragma unroll
          for (uint32_t n = 0; n < 8; ++n) tvv[n] = n == from ? max(tvv[n], rvv[n]) : tvv[n];
          o += kLdRemRec;
        }
      }
      // this.merge(copy): ORSet.merge of the keys, then ORMap.dryMerge over the merged keys
      bool live = false;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const uint32_t x = orset_merge_entry(d[n], td[n], cur[n], tvv[n]);
        dirty |= x != d[n];
        d[n] = x;
        live |= x != 0u;
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        vch |= tvv[n] > cur[n];
        cur[n] = max(cur[n], tvv[n]);
      }
      dch = true;
      const bool that = tval && (!was || tts > ts || (tts == ts && (trg >> 24) < (rg >> 24)));
      ts = !live ? 0 : that ? tts : ts;
      rg = !live ? 0u : that ? trg : rg;
#pragma unroll
      for (uint32_t n = 0; n < 8; ++n) dv[n] = n == from ? hi : dv[n];  // deltaVersions(from) = toSeqNr
    } else if (c == kLwPut || c == kLwRemove) {
      uint32_t ver = 0;
      const uint32_t key = arg & (AGX_ORSET_ELEMS - 1u);
      if (c == kLwPut) {  // ORSet.add of the key: vvector + node; birth dot (node -> new version)
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n)
          if (n == node) ver = cur[n] = cur[n] + 1u;
        if (ver == 0u && k == 0) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long version would not wrap
        vch = true;
      }
      sch = true;
      if (key == k) {
        if (c == kLwPut) {
          bool present = false, over;
#pragma unroll
          for (int n = 0; n < 8; ++n) present |= d[n] != 0u;
          ts = lww_clock(clock, now, present ? ts : 0, &over);
          if (over) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long timestamp would wrap
          rg = (node << 24) | (arg >> 6);
        } else {
          ts = 0;
          rg = 0u;
        }
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) d[n] = (c == kLwPut && n == node) ? ver : 0u;
        dirty = true;
      }
      // DeltaPropagationSelector.update: the next seqNr's ring entry, in the lane of its slot
      const uint32_t sq = ++ctr;
      if (sq > AGX_DELTA_LOG && k == 0) {
        bool lost = false;
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) lost |= n < m && n != node && sent[n] < sq - AGX_DELTA_LOG;
        if (lost) atomicOr(P.err, 1ull);  // kErrCapacity: the overwritten seqNr was not sent to every node
      }
      const uint32_t ptl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)ts, (int)key);
      const uint32_t pth = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)ts >> 32), (int)key);
      if ((sq % AGX_DELTA_LOG) == k) {
        const bool put = c == kLwPut;
        e[0] = sq;
        e[1] = lwd_tk(c, arg);
        e[2] = put ? ver : 0u;
        e[3] = put ? ((node << 24) | (arg >> 6)) : 0u;
        e[4] = put ? ptl : 0u;
        e[5] = put ? pth : 0u;
        e[6] = e[7] = 0u;
#pragma unroll
        for (int n = 0; n < 8; ++n) e[8 + n] = put ? 0u : cur[n];
        edirty = true;
      }
    } else if (c == kLwSnap && f) {  // snapshot row as lwwmap_merge_wave's, the deltaVersions behind the data
      const uint32_t hr = h++;
      if (hr < H.rows) {
        uint32_t* row = H.wrow(hr);
        uint32_t mk = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) mk |= d[n] ? 1u << n : 0u;
        const uint32_t cnt = __popc(mk);
        const uint32_t incl = wave_incl_sum(cnt);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        const uint64_t lm = __ballot(mk != 0u);
        uint32_t o = kOrRowDots + incl - cnt;
        const uint32_t go = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm & lt);
        const uint32_t dvo = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm);  // (<= 736: at most 512 dots, 64 live keys)
        reinterpret_cast<uint8_t*>(row + kOrRowMask)[k] = (uint8_t)mk;
#pragma unroll
        for (int n = 0; n < 8; ++n)
          if (d[n]) row[o++] = d[n];
        if (mk) {
          row[go] = (uint32_t)(uint64_t)ts;
          row[go + 1] = (uint32_t)((uint64_t)ts >> 32);
          row[go + 2] = rg;
        }
        if (k < AGX_CRDT_NODES) row[dvo + k] = lwd_pick(dv, k);
        if (k == 0) {
          *reinterpret_cast<uint4*>(row + kOrRowVV) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
          *reinterpret_cast<uint4*>(row + kOrRowVV + 4) = make_uint4(cur[4], cur[5], cur[6], cur[7]);
          row[kLwRowLen] = dvo + AGX_CRDT_NODES;
        }
      }
    } else if (c == kLdTick && na) {  // DeltaPropagationTick: one group row per slice node with unsent seqNrs
      const uint32_t sz = dl_slice_size(na), cnt = na <= sz ? na : sz;
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t x = dl_slice_node(node, na, sz, rr, i);
        const uint32_t j = lwd_pick(sent, x);
        if (ctr <= j) continue;
        const uint32_t hr = h++;
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) sent[n] = n == x ? ctr : sent[n];
        if (hr >= H.rows) continue;
        // ring slot k holds seqNr e[0]; its place in the group is pos = e[0] - (j + 1) if that is < ctr - j.
        // The masks below are in group order (bit p = place p): the lane masks rotated by the first slot.
        const uint32_t gc = min(ctr - j, AGX_DELTA_LOG), rot = (j + 1u) % AGX_DELTA_LOG;
        const uint32_t pos = (k - rot) % AGX_DELTA_LOG;
        const bool in = pos < gc;
        const uint32_t tk = in ? e[1] : 0u;
        const uint32_t tkp = (uint32_t)__shfl((int)tk, (int)((k + kWave - 1u) % kWave));  // the entry before / after in seqNr order
        const uint32_t tkn = (uint32_t)__shfl((int)tk, (int)((k + 1u) % kWave));
        const bool isput = (tk & 0xFFu) == 1u;
        const bool start = in && !(isput && pos > 0u && tkp == tk);               // opens an op of the group
        const bool last = in && !(isput && pos + 1u < gc && tkn == tk);            // its run's last entry: writes the op
        const uint64_t below = (1ull << pos) - 1ull;
        const uint32_t nops = (uint32_t)__popcll(__ballot(start));
        const uint64_t lp = lwd_rotr(__ballot(last && isput), rot), lr = lwd_rotr(__ballot(last && !isput), rot);
        // (lwd_group_ph calls a group of more than AGX_DELTA_LOG seqNrs a placeholder whatever this says of its last 64:
        // the two can disagree only in a run that has raised AGX_ECAPACITY, whose results are discarded)
        const bool ph = gc >= 2u && nops >= P.delta_max;
        uint32_t* row = H.wrow(hr);
        if (!ph && last) {
          uint32_t o = 12u + kLdPutRec * (uint32_t)__popcll(lp & below) + kLdRemRec * (uint32_t)__popcll(lr & below);
          row[o] = tk;
          if (isput) {
            row[o + 1] = e[2];
            row[o + 2] = e[3];
            row[o + 3] = e[4];
            row[o + 4] = e[5];
          } else {
#pragma unroll
            for (int n = 0; n < 8; ++n) row[o + 1 + n] = e[8 + n];
          }
        }
        if (k < AGX_CRDT_NODES) row[4 + k] = lwd_pick(dv, k);
        if (k == 0) {  // (rows are recycled: every field the receiver reads is written)
          row[0] = ph ? 0x80000000u : nops;
          row[1] = node;
          row[2] = j + 1u;
          row[3] = ctr;
          row[H.pw - 1] = 12u + (ph ? 0u : kLdPutRec * (uint32_t)__popcll(lp) + kLdRemRec * (uint32_t)__popcll(lr));
        }
      }
      rr += sz;
      sch = true;
    }
  }
  if (dirty) {
    se[0] = make_uint4(d[0], d[1], d[2], d[3]);
    se[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
  if (ts != ts0) *tp = ts;
  if (rg != rg0) *gp = rg;
  if (edirty) {
    rg4[0] = make_uint4(e[0], e[1], e[2], e[3]);
    rg4[1] = make_uint4(e[4], e[5], e[6], e[7]);
    rg4[2] = make_uint4(e[8], e[9], e[10], e[11]);
    rg4[3] = make_uint4(e[12], e[13], e[14], e[15]);
  }
  if (k == 0) {
    if (vch) {
      uint4* vo = reinterpret_cast<uint4*>(st + vw);
      vo[0] = make_uint4(cur[0], cur[1], cur[2], cur[3]);
      vo[1] = make_uint4(cur[4], cur[5], cur[6], cur[7]);
    }
    if (dch) {
      ev4[0] = make_uint4(dv[0], dv[1], dv[2], dv[3]);
      ev4[1] = make_uint4(dv[4], dv[5], dv[6], dv[7]);
    }
    if (sch) {
      ev4[2] = make_uint4(ctr, rr, sent[0], sent[1]);
      ev4[3] = make_uint4(sent[2], sent[3], sent[4], sent[5]);
      ev4[4] = make_uint4(sent[6], sent[7], 0u, 0u);
    }
  }
}

}  // namespace agx
