// agx_ormm.h — ORMultiMap replicas on the device (include/akka_gpu.h "ORMultiMap replicas"):
// ORMultiMap[A, B] = ORMap[A, ORSet[B]] over the 64-key universe, 8 values per key, withValueDeltas = false.
//
//   ORMultiMap.merge / put / remove                DD/ORMultiMap.scala:78-91,182-189,216-225
//   addBinding / removeBinding / replaceBinding    DD/ORMultiMap.scala:248-252,277-290,310-318
//   ORMap.updated / remove / merge                 DD/ORMap.scala:308-334,361-366,379-409 (dryMerge)
//   ORSet.add / remove / clear / merge             DD/ORSet.scala:339,380,404,427- (the key set and every
//                                                  value set are ORSets; orset_merge_entry per dot)
//
// An ORMultiMap engine holds ORMultiMap replicas only (variant V_ORMM) and follows the PNCounterMap wave
// path with code of its own: ormm_protocol (one lane per replica, inside k_bucket_apply) does the tells,
// the snapshot-row allocation in message order and the unhandled count, and lists the run;
// k_ormm_merge (one wave per replica, lane k = key k) then applies the run's state effects.
#pragma once
#include "agx_crdt.h"

namespace agx {

// data type code of a map engine's state gossip (payload >> 30; 3 = the engine's ORMap-based map)
constexpr uint32_t kMmType = 3u;
// Snapshot row (u32): the sparse ORSet form for the keys (kOrRow*: version vector, 64 mask bytes, the
// live key dots in (key, node) order), the dots section rounded up to a multiple of 4 u32, then the
// 72 u32 value set {version vector[8], dots[8 values][8 nodes]} of every key whose mask byte is
// non-zero, in key order: every block is 16-B aligned and moves as 18 x 16 B.  [kMmRowLen] holds the
// row's used length: a gossip that stays queued past the throughput cap has its row copied forward
// that far (bucket_finish).  Whatever a row's mask bytes say, a reader stays inside kMmRowMax: 64
// bytes of at most 8 bits each place a block at 32 + 512 + 72 x 63 at most.
constexpr uint32_t kMmRowLen = kOrRowDV;
constexpr uint32_t kMmSetU32 = AGX_ORMM_SET_U32;  // one key's value set, in the state and in a row
constexpr uint32_t kMmRowMax = kOrRowDots + AGX_ORSET_ELEMS * AGX_CRDT_NODES + kMmSetU32 * AGX_ORSET_ELEMS;
static_assert(kMmRowMax == 5152u, "ORMultiMap row: 32 header + 512 key dots + 64 x 72 value-set u32 at most");
static_assert(kMmRowMax == 2u * AGX_ORMM_WORDS, "the widest row is exactly the pitch derived from 2 x 2576 u32");
static_assert((AGX_ORSET_ELEMS * AGX_CRDT_NODES) % 4u == 0 && kOrRowDots % 4u == 0 && kMmSetU32 % 4u == 0,
              "the rounded dots section and every value-set block are 16-B aligned");
static_assert(kMmSetU32 == AGX_CRDT_NODES + AGX_ORMM_VALUES * AGX_CRDT_NODES && AGX_ORMM_VALUES == 8u && AGX_CRDT_NODES == 8u,
              "a value set: its version vector, then 8 values x 8 node dots");
static_assert(AGX_ORMM_WORDS == 2576u && AGX_ORMM_WORDS * 8u == 161u * 128u && AGX_ORMM_SET_WORD % 2u == 0 &&
                  AGX_ORMM_SET_WORD >= AGX_ORSET_WORDS &&
                  AGX_ORMM_WORDS == AGX_ORMM_SET_WORD + AGX_ORSET_ELEMS * (kMmSetU32 / 2u),
              "ORMultiMap state: 2576 u64 = 161 lines of 128 B; the ORSet words, padding, 64 x 36 words of value sets");

constexpr uint32_t kMmMerge = 1, kMmAdd = 2, kMmUnbind = 3, kMmPut = 4, kMmReplace = 5, kMmRemove = 6, kMmSnap = 7;
__device__ __forceinline__ uint32_t ormm_code(uint32_t sv, uint32_t pv) {
  if (is_wide(sv)) return (pv >> 30) == kMmType && !(pv & AGX_DELTA_ROW_BIT) ? kMmMerge : 0u;
  const uint32_t op = pv >> 24, arg = pv & 0xFFFFFFu;
  constexpr uint32_t kBind = AGX_ORSET_ELEMS * AGX_ORMM_VALUES;  // key | value << 6
  if (op == AGX_OP_ADD) return arg < kBind ? kMmAdd : 0u;
  if (op == AGX_OP_REMOVE_BINDING) return arg < kBind ? kMmUnbind : 0u;
  if (op == AGX_OP_PUT) return arg < (AGX_ORSET_ELEMS << AGX_ORMM_VALUES) ? kMmPut : 0u;  // key | mask << 6, mask < 256
  if (op == AGX_OP_REPLACE_BINDING) return arg < kBind * AGX_ORMM_VALUES ? kMmReplace : 0u;  // key | old << 6 | new << 9
  if (op == AGX_OP_REMOVE) return arg < AGX_ORSET_ELEMS ? kMmRemove : 0u;
  if (op == AGX_OP_GOSSIP) return kMmSnap;
  return 0u;
}

// phase A (per lane): the tells one message of an ORMultiMap replica will produce; *rows += its snapshot row
__device__ __forceinline__ uint32_t ormm_count(const DevParams& P, uint32_t src, uint32_t pay, uint32_t* rows) {
  if (is_wide(src) || (pay >> 24) != AGX_OP_GOSSIP) return 0;
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  *rows += f ? 1u : 0u;
  return f + ((pay & 0xFFFFFFu) > 0 ? 1u : 0u);
}

// phase B (per lane): tells and snapshot-row handles in message order; returns the unhandled count;
// *state_work: the run reads or writes the state (k_ormm_merge then walks it)
template <typename Emit, typename Src, typename Pay>
__device__ __forceinline__ uint32_t ormm_protocol(const DevParams& P, uint32_t self, uint32_t s0, uint32_t nd,
                                                  const Src& isrc, const Pay& ipay, uint32_t& row_cursor, Emit& em,
                                                  bool* state_work) {
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint32_t nunh = 0, nmod = 0;
  const uint32_t rc0 = row_cursor;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(s0 + q), pv = ipay(s0 + q);
    const uint32_t c = ormm_code(sv, pv);
    if (c == 0) {
      ++nunh;
      continue;
    }
    if (c != kMmSnap) {
      ++nmod;
      continue;
    }
    const uint32_t arg = pv & 0xFFFFFFu;
    if (f) {
      const uint32_t tagged = (kMmType << 30) | row_cursor++;
      for (uint32_t j = 0; j < f; ++j) em.wide(crdt_peer(P.gossip_seed, self, arg, j, P.n_global), tagged);
    }
    if (arg > 0) em(self, AGX_OP(AGX_OP_GOSSIP, arg - 1u));
  }
  *state_work = nmod != 0 || row_cursor != rc0;
  return nunh;
}

// One replica's run of nd messages (wave-uniform arguments, all 64 lanes converged), lane k = key k.
// Each lane holds its key's 8 key dots (2 x 16 B) and its value set (72 u32 = 18 x 16 B: the set's own
// version vector, then 8 values x 8 node dots), and the wave the key set's version vector; every load
// of the state is issued before any dependent work.  The messages are then applied in order from
// registers -- message q sees what messages < q left -- and key dots, value set and version vector are
// stored once at the end, each only if changed.  Snapshot rows from rc0 on.  The state is canonical (a
// key without a live key dot has 72 zero u32) and stays so, which is what lets the value rule of
// ORMap.dryMerge be one ORSet.merge: a side without the key contributes an empty set with a zero
// version vector, and merging with that is the identity.  A received row's value set is streamed value
// by value, 8 dots at a time against the two 8-entry version vectors.
template <typename Src, typename Pay>
__device__ __forceinline__ void ormm_merge_wave(const DevParams& P, const CrdtHeap& H, uint32_t l, uint32_t node,
                                                uint32_t nd, uint32_t rc0, const Src& isrc, const Pay& ipay) {
  static_assert(AGX_ORSET_ELEMS == kWave, "one lane per ORMultiMap key");
  constexpr uint32_t vw = AGX_ORSET_ELEMS * AGX_CRDT_NODES / 2;  // first word of the key set's version vector
  constexpr int NV = (int)AGX_ORMM_VALUES;
  constexpr int NB = (int)(kMmSetU32 / 4u);  // 18 x 16 B per value set
  const uint32_t k = lane_id();
  const uint64_t lt = (1ull << k) - 1ull;  // the lanes below this one
  const uint32_t f = P.n_global > 1 ? P.gossip_f : 0u;
  uint64_t* st = wide_state(P, l);
  uint4* se = reinterpret_cast<uint4*>(st + 4 * k);  // key k: 8 u32 key dots = 2 x 16 B
  const uint4* sv4 = reinterpret_cast<const uint4*>(st + vw);
  uint4* sc = reinterpret_cast<uint4*>(st + AGX_ORMM_SET_WORD + (kMmSetU32 / 2u) * k);  // key k: 72 u32 = 18 x 16 B
  const uint4 a0 = se[0], a1 = se[1], v0 = sv4[0], v1 = sv4[1];
  uint4 c4[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) c4[i] = sc[i];
  uint32_t d[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t vv0[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  uint32_t cur[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) cur[n] = vv0[n];
  uint32_t svv[8] = {c4[0].x, c4[0].y, c4[0].z, c4[0].w, c4[1].x, c4[1].y, c4[1].z, c4[1].w};  // the value set's vvector
  uint32_t e[NV][8];                                                                            // e[v][n]: dot of value v by node n
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const uint4 x = c4[2 + 2 * v], y = c4[3 + 2 * v];
    e[v][0] = x.x, e[v][1] = x.y, e[v][2] = x.z, e[v][3] = x.w;
    e[v][4] = y.x, e[v][5] = y.y, e[v][6] = y.z, e[v][7] = y.w;
  }
  bool dirty = false, sdirty = false;
  uint32_t h = rc0;
  for (uint32_t q = 0; q < nd; ++q) {
    const uint32_t sv = isrc(q), pv = ipay(q);
    const uint32_t c = ormm_code(sv, pv);
    const uint32_t arg = pv & 0xFFFFFFu;
    if (c == kMmMerge) {
      const uint32_t* row = H.row(pv & kHandleMask);
      // sparse row: key k's live key dots start after the earlier keys' (a wave prefix count); its value
      // set after the rounded dots section and the value sets of the earlier live keys
      const uint32_t rm = reinterpret_cast<const uint8_t*>(row + kOrRowMask)[k];
      const uint32_t rc = __popc(rm);
      const uint32_t incl = wave_incl_sum(rc);
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
      uint32_t ro = kOrRowDots + incl - rc;
      const uint32_t go = kOrRowDots + ((tot + 3u) & ~3u) + kMmSetU32 * (uint32_t)__popcll(__ballot(rm != 0u) & lt);
      const uint4 va = *reinterpret_cast<const uint4*>(row + kOrRowVV), vb = *reinterpret_cast<const uint4*>(row + kOrRowVV + 4);
      const uint4* rs4 = reinterpret_cast<const uint4*>(row + go);  // (go + 72 <= kMmRowMax <= the row pitch)
      const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
      const uint4 ra = rm ? rs4[0] : z4, rb = rm ? rs4[1] : z4;
      uint32_t r[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) r[n] = (rm >> n) & 1u ? row[ro++] : 0u;
      const uint32_t rvv[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
      const uint32_t rsv[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};  // the row's value-set vvector
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
      // ORMap.dryMerge over the merged keys: both sides -> ORSet.merge of the value sets with their own
      // version vectors; one side -> that side's set (the other side is all zero: canonical form); a key
      // that left the merged key set -> nothing
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const uint4 x = rm ? rs4[2 + 2 * v] : z4, y = rm ? rs4[3 + 2 * v] : z4;
        const uint32_t g[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          const uint32_t o = live ? orset_merge_entry(e[v][n], g[n], svv[n], rsv[n]) : 0u;
          sdirty |= o != e[v][n];
          e[v][n] = o;
        }
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const uint32_t o = live ? max(svv[n], rsv[n]) : 0u;
        sdirty |= o != svv[n];
        svv[n] = o;
      }
    } else if (c == kMmAdd || c == kMmUnbind || c == kMmPut || c == kMmReplace || c == kMmRemove) {
      const uint32_t key = arg & (AGX_ORSET_ELEMS - 1u);
      const uint32_t va = (arg >> 6) & 7u, vb = (arg >> 9) & 7u;  // value (old value), new value of a replace
      const uint32_t mask = c == kMmPut ? arg >> 6 : c == kMmAdd ? 1u << va : c == kMmReplace ? 1u << vb : 0u;  // values added
      const bool same = c == kMmReplace && va == vb;  // replaceBinding(old == new) returns `this`
      // ORMap.updated does keys.add(node, key): vvector + node, once per updated (a replace is two)
      const uint32_t nup = c == kMmRemove || same ? 0u : c == kMmReplace ? 2u : 1u;
      uint32_t ver = 0;
      if (nup) {
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n)
          if (n == node) {
            if (cur[n] > 0xFFFFFFFFu - nup && k == 0) atomicOr(P.err, 2ull);  // kErrRange: the reference's Long version would not wrap
            ver = cur[n] = cur[n] + nup;
          }
      }
      if (key == k && !same) {
        if (c == kMmRemove) {  // ORMap.remove: values - key
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int n = 0; n < 8; ++n) e[v][n] = 0u;
        } else {
          // the present set (or ORSet.empty: 72 zeros) modified: put clears first, removeBinding drops the
          // value's dots; every added value takes the set's next version at node as its one dot
          const uint32_t drop = c == kMmPut ? 0xFFu : c == kMmUnbind ? 1u << va : 0u;
          uint32_t sver = 0;
#pragma unroll
          for (uint32_t n = 0; n < 8; ++n)
            if (n == node) sver = svv[n];
          if (sver > 0xFFFFFFFFu - (uint32_t)__popc(mask)) atomicOr(P.err, 2ull);  // kErrRange: a value set's version
#pragma unroll
          for (uint32_t v = 0; v < (uint32_t)NV; ++v) {
            const bool add = (mask >> v) & 1u;
            if (add) ++sver;  // (ascending value index)
            if (add || ((drop >> v) & 1u)) {
#pragma unroll
              for (uint32_t n = 0; n < 8; ++n) e[v][n] = add && n == node ? sver : 0u;
            }
          }
          if (c == kMmReplace) {  // ... then removeBinding(old)
#pragma unroll
            for (uint32_t v = 0; v < (uint32_t)NV; ++v)
              if (v == va) {
#pragma unroll
                for (uint32_t n = 0; n < 8; ++n) e[v][n] = 0u;
              }
          }
#pragma unroll
          for (uint32_t n = 0; n < 8; ++n)
            if (n == node) svv[n] = sver;
        }
        // removeBinding that leaves the set empty is followed by ORMap.remove(node, key)
        bool gone = c == kMmRemove;
        if (c == kMmUnbind) {
          uint32_t any = 0;
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int n = 0; n < 8; ++n) any |= e[v][n];
          gone = any == 0u;
        }
        if (gone) {
#pragma unroll
          for (int n = 0; n < 8; ++n) svv[n] = 0u;
        }
#pragma unroll
        for (uint32_t n = 0; n < 8; ++n) d[n] = (!gone && n == node) ? ver : 0u;
        dirty = true;
        sdirty = true;
      }
    } else if (c == kMmSnap && f) {  // snapshot row: key k per lane, the vvector and the length from lane 0
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
        const uint32_t go = cb + kMmSetU32 * (uint32_t)__popcll(lm & lt);
        reinterpret_cast<uint8_t*>(row + kOrRowMask)[k] = (uint8_t)m;
#pragma unroll
        for (int n = 0; n < 8; ++n)
          if (d[n]) row[o++] = d[n];
        if (m) {  // (go + 72 <= kMmRowMax <= the row pitch: at most 512 key dots and 64 live keys)
          uint4* wc = reinterpret_cast<uint4*>(row + go);
          wc[0] = make_uint4(svv[0], svv[1], svv[2], svv[3]);
          wc[1] = make_uint4(svv[4], svv[5], svv[6], svv[7]);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            wc[2 + 2 * v] = make_uint4(e[v][0], e[v][1], e[v][2], e[v][3]);
            wc[3 + 2 * v] = make_uint4(e[v][4], e[v][5], e[v][6], e[v][7]);
          }
        }
        if (k == 0) {
          *reinterpret_cast<uint4*>(row + kOrRowVV) = make_uint4(cur[0], cur[1], cur[2], cur[3]);
          *reinterpret_cast<uint4*>(row + kOrRowVV + 4) = make_uint4(cur[4], cur[5], cur[6], cur[7]);
          row[kMmRowLen] = cb + kMmSetU32 * (uint32_t)__popcll(lm);
        }
      }
    }
  }
  if (dirty) {
    se[0] = make_uint4(d[0], d[1], d[2], d[3]);
    se[1] = make_uint4(d[4], d[5], d[6], d[7]);
  }
  if (sdirty) {
    sc[0] = make_uint4(svv[0], svv[1], svv[2], svv[3]);
    sc[1] = make_uint4(svv[4], svv[5], svv[6], svv[7]);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      sc[2 + 2 * v] = make_uint4(e[v][0], e[v][1], e[v][2], e[v][3]);
      sc[3 + 2 * v] = make_uint4(e[v][4], e[v][5], e[v][6], e[v][7]);
    }
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
