// agx_pncmap.h — PNCounterMap replicas on the device (include/akka_gpu.h "PNCounterMap replicas"):
// PNCounterMap[A] = ORMap[A, PNCounter] over the 64-key universe.
//
//   PNCounterMap.increment / decrement   DD/PNCounterMap.scala:105-106,139-141
//   ORMap.updated / remove / merge       DD/ORMap.scala:308-334,361-366,379-409 (dryMerge)
//   PNCounter.change / merge             DD/PNCounter.scala:173-178,180-183
//   ORSet.add / remove / merge           as agx_crdt.h (the key set is an ORSet, bit for bit)
//
// A PNCounterMap engine holds PNCounterMap replicas only (variant V_PNCMAP) and follows the LWWMap wave
// path with code of its own: pncmap_protocol (one lane per replica, inside k_bucket_apply) does the
// tells, the snapshot-row allocation in message order and the unhandled count, and lists the run;
// k_pncmap_merge (one wave per replica, lane k = key k) then applies the run's state effects.
#pragma once
#include "agx_crdt.h"

namespace agx {

// data type code of a map engine's state gossip (payload >> 30; 0..2 = GCounter, PNCounter, ORSet;
// 3 = the engine's ORMap-based map: an engine holds one map kind only)
constexpr uint32_t kPnType = 3u;
// Snapshot row (u32): the sparse ORSet form (kOrRow*: version vector, 64 mask bytes, the live dots
// in (key, node) order), the dots section rounded up to a multiple of 4 u32, then the 16 u64 slots
// {increments[8], decrements[8]} of every key whose mask byte is non-zero, in key order: every
// counter block is 16-B aligned.  [kPnRowLen] holds the row's used length: a gossip that stays
// queued past the throughput cap has its row copied forward that far (bucket_finish).
constexpr uint32_t kPnRowLen = kOrRowDV;
constexpr uint32_t kPnKeyU32 = 2u * AGX_PNCOUNTER_WORDS;  // one key's counters in a row
constexpr uint32_t kPnRowMax = kOrRowDots + AGX_ORSET_ELEMS * AGX_CRDT_NODES + kPnKeyU32 * AGX_ORSET_ELEMS;
static_assert(kPnRowMax == 2592u, "PNCounterMap row: 32 header + 512 dots + 64 x 32 counter u32 at most");
static_assert((AGX_ORSET_ELEMS * AGX_CRDT_NODES) % 4u == 0 && kOrRowDots % 4u == 0 && kPnKeyU32 % 4u == 0,
              "the rounded dots section and every counter block are 16-B aligned");
static_assert(AGX_PNCMAP_WORDS == 1296u && AGX_PNCMAP_WORDS * 8u == 81u * 128u && AGX_PNCMAP_CTR_WORD % 16u == 0 &&
                  AGX_PNCMAP_CTR_WORD >= AGX_ORSET_WORDS &&
                  AGX_PNCMAP_WORDS == AGX_PNCMAP_CTR_WORD + AGX_ORSET_ELEMS * AGX_PNCOUNTER_WORDS,
              "PNCounterMap state: 1296 u64 = 81 lines of 128 B; the ORSet words, padding to a line, 64 x 16 slots");

constexpr uint32_t kPnMerge = 1, kPnInc = 2, kPnDec = 3, kPnRemove = 4, kPnSnap = 5;
__device__ __forceinline__ uint32_t pncmap_code(uint32_t sv, uint32_t pv) {
  if (is_wide(sv)) return (pv >> 30) == kPnType && !(pv & AGX_DELTA_ROW_BIT) ? kPnMerge : 0u;
  const uint32_t op = pv >> 24, arg = pv & 0xFFFFFFu;
  if (op == AGX_OP_INCREMENT) return kPnInc;  // (key = arg & 63, n = arg >> 6: every argument is a count)
  if (op == AGX_OP_DECREMENT) return kPnDec;
  if (op == AGX_OP_REMOVE) return arg < AGX_ORSET_ELEMS ? kPnRemove : 0u;
  if (op == AGX_OP_GOSSIP) return kPnSnap;
  return 0u;
}

// phase A (per lane): the tells one message of a PNCounterMap replica will produce; *rows += its snapshot row
__device__ __forceinline__ uint32_t pncmap_count(const DevParams& P, uint32_t src, uint32_t pay, uint32_t* rows) {
  if (is_wide(src) || (pay >> 24) != AGX_OP_GOSSIP) return 0;
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  *rows += f ? 1u : 0u;
  return f + ((pay & 0xFFFFFFu) > 0 ? 1u : 0u);
}

// phase B (per lane): tells and snapshot-row handles in message order; returns the unhandled count;
// *state_work: the run reads or writes the state (k_pncmap_merge then walks it)
template <typename Emit, typename Src, typename Pay>
__device__ __forceinline__ uint32_t pncmap_protocol(const DevParams& P, uint32_t self, uint32_t s0, uint32_t nd,
                                                    const Src& isrc, const Pay& ipay, uint32_t& row_cursor, Emit& em,
                                                    bool* state_work) {
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint32_t nunh = 0, nmod = 0;
  const uint32_t rc0 = row_cursor;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(s0 + q), pv = ipay(s0 + q);
    const uint32_t c = pncmap_code(sv, pv);
    if (c == 0) {
      ++nunh;
      continue;
    }
    if (c != kPnSnap) {
      ++nmod;
      continue;
    }
    const uint32_t arg = pv & 0xFFFFFFu;
    if (f) {
      const uint32_t tagged = (kPnType << 30) | row_cursor++;
      for (uint32_t j = 0; j < f; ++j) em.wide(crdt_peer(P.gossip_seed, self, arg, j, P.n_global), tagged);
    }
    if (arg > 0) em(self, AGX_OP(AGX_OP_GOSSIP, arg - 1u));
  }
  *state_work = nmod != 0 || row_cursor != rc0;
  return nunh;
}

__device__ __forceinline__ uint64_t pn_u64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// One replica's run of nd messages (wave-uniform arguments, all 64 lanes converged), lane k = key k.
// Each lane holds its key's 8 dots (2 x 16 B) and its 16 slots (one aligned 128-B line, 8 x 16 B), and
// the wave the version vector; every load of the state is issued before any dependent work.  The
// messages are then applied in order from registers -- message q sees what messages < q left -- and
// dots, slots and version vector are stored once at the end, each only if changed.  Snapshot rows from
// rc0 on.  The state is canonical (a key without a live dot has 16 zero slots) and stays so, which is
// what lets the value rule of ORMap.dryMerge be one slot-wise maximum: a side without the key
// contributes zeros.
template <typename Src, typename Pay>
__device__ __forceinline__ void pncmap_merge_wave(const DevParams& P, const CrdtHeap& H, uint32_t l, uint32_t node,
                                                  uint32_t nd, uint32_t rc0, const Src& isrc, const Pay& ipay) {
  static_assert(AGX_ORSET_ELEMS == kWave, "one lane per PNCounterMap key");
  constexpr uint32_t vw = AGX_ORSET_ELEMS * AGX_CRDT_NODES / 2;  // first vvector word
  constexpr int NS = (int)AGX_PNCOUNTER_WORDS;                     // 16 slots per key
  const uint32_t k = lane_id();
  const uint64_t lt = (1ull << k) - 1ull;  // the lanes below this one
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint64_t* st = wide_state(P, l);
  uint4* se = reinterpret_cast<uint4*>(st + 4 * k);  // key k: 8 u32 dots = 2 x 16 B
  const uint4* sv4 = reinterpret_cast<const uint4*>(st + vw);
  uint4* sc = reinterpret_cast<uint4*>(st + AGX_PNCMAP_CTR_WORD + NS * k);  // key k: 16 u64 slots = one 128-B line
  const uint4 a0 = se[0], a1 = se[1], v0 = sv4[0], v1 = sv4[1];
  uint4 c4[NS / 2];
#pragma unroll
  for (int i = 0; i < NS / 2; ++i) c4[i] = sc[i];
  uint32_t d[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t vv0[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  uint32_t cur[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) cur[n] = vv0[n];
  uint64_t s[NS];
#pragma unroll
  for (int i = 0; i < NS / 2; ++i) {
    s[2 * i] = pn_u64(c4[i].x, c4[i].y);
    s[2 * i + 1] = pn_u64(c4[i].z, c4[i].w);
  }
  bool dirty = false, sdirty = false;
  uint32_t h = rc0;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(q), pv = ipay(q);
    const uint32_t c = pncmap_code(sv, pv);
    const uint32_t arg = pv & 0xFFFFFFu;
    if (c == kPnMerge) {
      const uint32_t* row = H.row(pv & kHandleMask);
      // sparse row: key k's live dots start after the earlier keys' (a wave prefix count); its counters
      // after the rounded dots section and the counters of the earlier live keys
      const uint32_t rm = reinterpret_cast<const uint8_t*>(row + kOrRowMask)[k];
      const uint32_t rc = __popc(rm);
      const uint32_t incl = wave_incl_sum(rc);
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
      uint32_t ro = kOrRowDots + incl - rc;
      const uint32_t go = kOrRowDots + ((tot + 3u) & ~3u) + kPnKeyU32 * (uint32_t)__popcll(__ballot(rm != 0u) & lt);
      const uint4 va = *reinterpret_cast<const uint4*>(row + kOrRowVV), vb = *reinterpret_cast<const uint4*>(row + kOrRowVV + 4);
      const uint4* rc4 = reinterpret_cast<const uint4*>(row + go);
      uint4 g4[NS / 2];
#pragma unroll
      for (int i = 0; i < NS / 2; ++i) g4[i] = rm ? rc4[i] : make_uint4(0u, 0u, 0u, 0u);
      uint32_t r[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) r[n] = (rm >> n) & 1u ? row[ro++] : 0u;
      const uint32_t rvv[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
      bool live = false;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const uint32_t o = orset_merge_entry(d[n], r[n], cur[n], rvv[n]);
        dirty |= o != d[n];
        d[n] = o;
        live |= o != 0u;
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) cur[n] = max(cur[n], rvv[n]);
      // ORMap.dryMerge over the merged keys: both sides -> PNCounter.merge, the slot-wise maximum; one
      // side -> that side's counter (the other side's slots are zero: canonical form); a key that left
      // the merged set -> nothing
#pragma unroll
      for (int i = 0; i < NS / 2; ++i) {
        const uint64_t x = pn_u64(g4[i].x, g4[i].y), y = pn_u64(g4[i].z, g4[i].w);
        const uint64_t n0 = !live ? 0ull : max(s[2 * i], x), n1 = !live ? 0ull : max(s[2 * i + 1], y);
        sdirty |= n0 != s[2 * i] || n1 != s[2 * i + 1];
        s[2 * i] = n0;
        s[2 * i + 1] = n1;
      }
    } else if (c == kPnInc || c == kPnDec || c == kPnRemove) {
      uint32_t ver = 0;
      if (c != kPnRemove) {  // ORSet.add of the key: vvector + node; birth dot (node -> new version)
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n)
          if (n == node) ver = cur[n] = cur[n] + 1u;
        if (ver == 0u && k == 0) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long version would not wrap
      }
      if ((arg & (AGX_ORSET_ELEMS - 1u)) == k) {
        if (c != kPnRemove) {  // ORMap.updated: the present counter (or a fresh one: 16 zeros), PNCounter.change
          const uint64_t by = arg >> 6;
          const uint32_t w = (c == kPnDec ? AGX_CRDT_NODES : 0u) + node;
#pragma unroll
          for (uint32_t i = 0; i < (uint32_t)NS; ++i)
            if (i == w) {
              const uint64_t v = s[i] + by;
              if (v < by) atomicOr(P.err, 2ull);  // kErrRange: the reference's BigInt slot would not wrap
              sdirty |= by != 0ull;
              s[i] = v;
            }
        } else {  // ORMap.remove: values - key
#pragma unroll
          for (int i = 0; i < NS; ++i) {
            sdirty |= s[i] != 0ull;
            s[i] = 0ull;
          }
        }
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) d[n] = (c != kPnRemove && n == node) ? ver : 0u;
        dirty = true;
      }
    } else if (c == kPnSnap && f) {  // snapshot row: key k per lane, the vvector and the length from lane 0
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
        const uint32_t cb = kOrRowDots + ((tot + 3u) & ~3u);
        const uint32_t go = cb + kPnKeyU32 * (uint32_t)__popcll(lm & lt);
        reinterpret_cast<uint8_t*>(row + kOrRowMask)[k] = (uint8_t)m;
#pragma unroll
        for (int n = 0; n < 8; ++n)
          if (d[n]) row[o++] = d[n];
        if (m) {  // (go + 32 <= kPnRowMax <= the row pitch: at most 512 dots and 64 live keys)
          uint4* wc = reinterpret_cast<uint4*>(row + go);
#pragma unroll
          for (int i = 0; i < NS / 2; ++i)
            wc[i] = make_uint4((uint32_t)s[2 * i], (uint32_t)(s[2 * i] >> 32), (uint32_t)s[2 * i + 1], (uint32_t)(s[2 * i + 1] >> 32));
        }
        if (k == 0) {
          *reinterpret_cast<uint4*>(row + kOrRowVV) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
          *reinterpret_cast<uint4*>(row + kOrRowVV + 4) = make_uint4(cur[4], cur[5], cur[6], cur[7]);
          row[kPnRowLen] = cb + kPnKeyU32 * (uint32_t)__popcll(lm);
        }
      }
    }
  }
  if (dirty) {
    se[0] = make_uint4(d[0], d[1], d[2], d[3]);
    se[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
  if (sdirty) {
#pragma unroll
    for (int i = 0; i < NS / 2; ++i)
      sc[i] = make_uint4((uint32_t)s[2 * i], (uint32_t)(s[2 * i] >> 32), (uint32_t)s[2 * i + 1], (uint32_t)(s[2 * i + 1] >> 32));
  }
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
