// agx_lwwmap.h — LWWMap replicas on the device (include/akka_gpu.h "LWWMap replicas"):
// LWWMap[A, B] = ORMap[A, LWWRegister[B]] over the 64-key universe.
//
//   LWWMap.put / remove / merge      DD/LWWMap.scala:144-150,175-187
//   ORMap.put / remove / merge       DD/ORMap.scala:254-265,361-366,379-409 (dryMerge)
//   LWWRegister clocks               DD/LWWRegister.scala:24-38
//   LWWRegister.withValue / merge    DD/LWWRegister.scala:192-199
//   ORSet.add / remove / merge       as agx_crdt.h (the key set is an ORSet, bit for bit)
//
// An LWWMap engine holds LWWMap replicas only (variant V_LWWMAP) and follows the ORSet wave path
// with code of its own: lwwmap_protocol (one lane per replica, inside k_bucket_apply) does the
// tells, the snapshot-row allocation in message order and the unhandled count, and lists the run;
// k_lwwmap_merge (one wave per replica, lane k = key k) then applies the run's state effects.
#pragma once
#include "agx_crdt.h"

namespace agx {

// data type code of an LWWMap state gossip (payload >> 30; 0..2 = GCounter, PNCounter, ORSet)
constexpr uint32_t kLwType = 3u;
// Snapshot row (u32): the sparse ORSet form (kOrRow*: version vector, 64 mask bytes, the live dots
// in (key, node) order), then {timestamp lo, hi, node << 24 | value} of every key whose mask byte is
// non-zero, in key order.  [kLwRowLen] holds the row's used length: a gossip that stays queued past
// the throughput cap has its row copied forward that far (bucket_finish).
constexpr uint32_t kLwRowLen = kOrRowDV;
constexpr uint32_t kLwRowMax = kOrRowDots + AGX_ORSET_ELEMS * AGX_CRDT_NODES + 3u * AGX_ORSET_ELEMS;
static_assert(kLwRowMax == 736u, "LWWMap row: 32 header + 512 dots + 192 register u32 at most");
static_assert(AGX_LWWMAP_TS_WORD == AGX_ORSET_WORDS && AGX_LWWMAP_REG_U32 == 2u * (AGX_LWWMAP_TS_WORD + AGX_ORSET_ELEMS) &&
                  AGX_LWWMAP_WORDS == AGX_LWWMAP_REG_U32 / 2u + AGX_ORSET_ELEMS / 2u,
              "LWWMap state: the ORSet words, 64 timestamps, 64 u32 registers");

constexpr uint32_t kLwMerge = 1, kLwPut = 2, kLwRemove = 3, kLwSnap = 4;
__device__ __forceinline__ uint32_t lwwmap_code(uint32_t sv, uint32_t pv) {
  if (is_wide(sv)) return (pv >> 30) == kLwType && !(pv & AGX_DELTA_ROW_BIT) ? kLwMerge : 0u;
  const uint32_t op = pv >> 24, arg = pv & 0xFFFFFFu;
  if (op == AGX_OP_PUT) return kLwPut;  // (key = arg & 63, value = arg >> 6: every argument is a put)
  if (op == AGX_OP_REMOVE) return arg < AGX_ORSET_ELEMS ? kLwRemove : 0u;
  if (op == AGX_OP_GOSSIP) return kLwSnap;
  return 0u;
}

// phase A (per lane): the tells one message of an LWWMap replica will produce; *rows += its snapshot row
__device__ __forceinline__ uint32_t lwwmap_count(const DevParams& P, uint32_t src, uint32_t pay, uint32_t* rows) {
  if (is_wide(src) || (pay >> 24) != AGX_OP_GOSSIP) return 0;
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  *rows += f ? 1u : 0u;
  return f + ((pay & 0xFFFFFFu) > 0 ? 1u : 0u);
}

// phase B (per lane): tells and snapshot-row handles in message order; returns the unhandled count;
// *state_work: the run reads or writes the state (k_lwwmap_merge then walks it)
template <typename Emit, typename Src, typename Pay>
__device__ __forceinline__ uint32_t lwwmap_protocol(const DevParams& P, uint32_t self, uint32_t s0, uint32_t nd,
                                                    const Src& isrc, const Pay& ipay, uint32_t& row_cursor, Emit& em,
                                                    bool* state_work) {
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint32_t nunh = 0, nmod = 0;
  const uint32_t rc0 = row_cursor;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(s0 + q), pv = ipay(s0 + q);
    const uint32_t c = lwwmap_code(sv, pv);
    if (c == 0) {
      ++nunh;
      continue;
    }
    if (c != kLwSnap) {
      ++nmod;
      continue;
    }
    const uint32_t arg = pv & 0xFFFFFFu;
    if (f) {
      const uint32_t tagged = (kLwType << 30) | row_cursor++;
      for (uint32_t j = 0; j < f; ++j) em.wide(crdt_peer(P.gossip_seed, self, arg, j, P.n_global), tagged);
    }
    if (arg > 0) em(self, AGX_OP(AGX_OP_GOSSIP, arg - 1u));
  }
  *state_work = nmod != 0 || row_cursor != rc0;
  return nunh;
}

// LWWRegister clock: the new timestamp of a register at `ts` written at logical time `now`
// (|now| < 2^63: base < 2^62, the step counter < 2^32).  *over: the reference's Long would wrap.
__device__ __forceinline__ int64_t lww_clock(uint32_t clock, int64_t now, int64_t ts, bool* over) {
  if (clock == AGX_LWW_CLOCK_REVERSE) {
    *over = ts == INT64_MIN;
    const int64_t t = (int64_t)((uint64_t)ts - 1ull);
    return -now < t ? -now : t;
  }
  *over = ts == INT64_MAX;
  const int64_t t = (int64_t)((uint64_t)ts + 1ull);
  return now > t ? now : t;
}

// One replica's run of nd messages (wave-uniform arguments, all 64 lanes converged), lane k = key k.
// Each lane holds its key's 8 dots (32 B), timestamp (8 B) and register word (4 B), and the wave the
// version vector; every load of the state is issued before any dependent work.  The messages are then
// applied in order from registers -- message q sees what messages < q left -- and dots, timestamp and
// register are stored once at the end, each only if changed.  Snapshot rows from rc0 on.
template <typename Src, typename Pay>
__device__ __forceinline__ void lwwmap_merge_wave(const DevParams& P, const CrdtHeap& H, uint32_t l, uint32_t node,
                                                  uint32_t nd, uint32_t rc0, uint32_t clock, int64_t now,
                                                  const Src& isrc, const Pay& ipay) {
  static_assert(AGX_ORSET_ELEMS == kWave, "one lane per LWWMap key");
  constexpr uint32_t vw = AGX_ORSET_ELEMS * AGX_CRDT_NODES / 2;  // first vvector word
  const uint32_t k = lane_id();
  const uint64_t lt = (1ull << k) - 1ull;  // the lanes below this one
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint64_t* st = wide_state(P, l);
  uint4* se = reinterpret_cast<uint4*>(st + 4 * k);  // key k: 8 u32 dots = 2 x 16 B
  const uint4* sv4 = reinterpret_cast<const uint4*>(st + vw);
  int64_t* tp = reinterpret_cast<int64_t*>(st + AGX_LWWMAP_TS_WORD) + k;
  uint32_t* gp = reinterpret_cast<uint32_t*>(st) + AGX_LWWMAP_REG_U32 + k;
  const uint4 a0 = se[0], a1 = se[1], v0 = sv4[0], v1 = sv4[1];
  const int64_t ts0 = *tp;
  const uint32_t rg0 = *gp;
  uint32_t d[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t vv0[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  uint32_t cur[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) cur[n] = vv0[n];
  int64_t ts = ts0;
  uint32_t rg = rg0;
  bool dirty = false;
  uint32_t h = rc0;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(q), pv = ipay(q);
    const uint32_t c = lwwmap_code(sv, pv);
    const uint32_t arg = pv & 0xFFFFFFu;
    if (c == kLwMerge) {
      const uint32_t* row = H.row(pv & kHandleMask);
      // sparse row: key k's live dots start after the earlier keys' (a wave prefix count); its register
      // after all dots and the registers of the earlier live keys
      const uint32_t rm = reinterpret_cast<const uint8_t*>(row + kOrRowMask)[k];
      const uint32_t rc = __popc(rm);
      const uint32_t incl = wave_incl_sum(rc);
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
      uint32_t ro = kOrRowDots + incl - rc;
      const uint32_t go = kOrRowDots + tot + 3u * (uint32_t)__popcll(__ballot(rm != 0u) & lt);
      const uint4 va = *reinterpret_cast<const uint4*>(row + kOrRowVV), vb = *reinterpret_cast<const uint4*>(row + kOrRowVV + 4);
      uint32_t r[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) r[n] = (rm >> n) & 1u ? row[ro++] : 0u;
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
      for (int n = 0; n < 8; ++n) cur[n] = max(cur[n], rvv[n]);
      // ORMap.dryMerge over the merged keys: both sides -> LWWRegister.merge; one side -> that side's
      // register; a key that left the merged set -> no register
      const int64_t rts = (int64_t)(((uint64_t)rth << 32) | rtl);
      const bool that = rm != 0u && (!was || rts > ts || (rts == ts && (rrg >> 24) < (rg >> 24)));
      ts = !live ? 0 : that ? rts : ts;
      rg = !live ? 0u : that ? rrg : rg;
    } else if (c == kLwPut || c == kLwRemove) {
      uint32_t ver = 0;
      if (c == kLwPut) {  // ORSet.add of the key: vvector + node; birth dot (node -> new version)
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n)
          if (n == node) ver = cur[n] = cur[n] + 1u;
        if (ver == 0u && k == 0) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long version would not wrap
      }
      if ((arg & (AGX_ORSET_ELEMS - 1u)) == k) {
        if (c == kLwPut) {  // LWWMap.put: withValue on the present register, a fresh one otherwise
          bool present = false, over;
#pragma unroll
          for (int n = 0; n < 8; ++n) present |= d[n] != 0u;
          ts = lww_clock(clock, now, present ? ts : 0, &over);
          if (over) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long timestamp would wrap
          rg = (node << 24) | (arg >> 6);
        } else {  // ORMap.remove: values - key
          ts = 0;
          rg = 0u;
        }
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) d[n] = (c == kLwPut && n == node) ? ver : 0u;
        dirty = true;
      }
    } else if (c == kLwSnap && f) {  // snapshot row: key k per lane, the vvector and the length from lane 0
      const uint32_t hr = h++;
      if (hr < H.rows) {
        uint32_t* row = H.wrow(hr);
        uint32_t m = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) m |= d[n] ? 1u << n : 0u;
        const uint32_t cnt = __popc(m);
        const uint32_t incl = wave_incl_sum(cnt);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        const uint64_t lm = __ballot(m != 0u);
        uint32_t o = kOrRowDots + incl - cnt;
        const uint32_t go = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm & lt);
        reinterpret_cast<uint8_t*>(row + kOrRowMask)[k] = (uint8_t)m;
#pragma unroll
        for (int n = 0; n < 8; ++n)
          if (d[n]) row[o++] = d[n];
        if (m) {  // (go + 2 < kLwRowMax <= the row pitch: at most 512 dots and 64 live keys)
          row[go] = (uint32_t)(uint64_t)ts;
          row[go + 1] = (uint32_t)((uint64_t)ts >> 32);
          row[go + 2] = rg;
        }
        if (k == 0) {
          *reinterpret_cast<uint4*>(row + kOrRowVV) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
          *reinterpret_cast<uint4*>(row + kOrRowVV + 4) = make_uint4(cur[4], cur[5], cur[6], cur[7]);
          row[kLwRowLen] = kOrRowDots + tot + 3u * (uint32_t)__popcll(lm);
        }
      }
    }
  }
  if (dirty) {
    se[0] = make_uint4(d[0], d[1], d[2], d[3]);
    se[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
  if (ts != ts0) *tp = ts;
  if (rg != rg0) *gp = rg;
  bool vch = false;
#pragma unroll
  for (int n = 0; n < 8; ++n) vch |= cur[n] != vv0[n];
  if (vch && k == 0) {
    uint4* vo = reinterpret_cast<uint4*>(st + vw);
    vo[0] = make_uint4(cur[0], cur[1], cur[2], cur[3]);
    vo[1] = make_uint4(cur[4], cur[5], cur[6], cur[7]);
  }
}

}  // namespace agx
