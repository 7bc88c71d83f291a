// agx_apply.hip — k_bucket_apply instantiations of one variant group (agx_variants.h).
// Built once per group with -DAGX_VGROUP=g; every unit exports its group's launches as one GroupLaunch
// (agx_group_<g>(), a host function: a const object would be emitted for the device too), and the unit of
// group 0 also holds the public launchers, which route a variant id to its group.
#include <hip/hip_runtime.h>

#include "agx_variants.h"

#ifndef AGX_VGROUP
#error "build agx_apply.hip with -DAGX_VGROUP=<group>"
#endif

#define AGX_CAT2(a, b) a##b
#define AGX_CAT(a, b) AGX_CAT2(a, b)

namespace agx {

// the launches of one group's variants (hipErrorInvalidValue for a variant of another group)
struct GroupLaunch {
  hipError_t (*apply)(uint32_t vid, uint32_t mode, bool skew, dim3, hipStream_t, const BucketArgs&);
  hipError_t (*feature)(uint32_t vid, uint32_t mode, uint32_t km_flags, bool prio, dim3, hipStream_t, const BucketArgs&);
  hipError_t (*tiny)(uint32_t vid, dim3, hipStream_t, const BucketArgs&);
  hipError_t (*dense)(uint32_t vid, uint32_t mode, dim3, hipStream_t, const BucketArgs&);
  hipError_t (*ring)(uint32_t vid, bool tiny, dim3, hipStream_t, const BucketArgs&, const RingArgs&);
  hipError_t (*persist_occupancy)(uint32_t vid, int*);
};
#define AGX_GROUPS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
static_assert(kVGroups == 13, "AGX_GROUPS names every group");
#define AGX_GROUP_DECL(g) const GroupLaunch& agx_group_##g();
AGX_GROUPS(AGX_GROUP_DECL)

namespace {

template <uint32_t V>
hipError_t launch_v(uint32_t mode, bool skew, dim3 g, hipStream_t s, const BucketArgs& ba) {
  constexpr bool W = kVariants[V].wide;
  constexpr uint32_t M = kVariants[V].km;
  const dim3 blk(kBThreads);
  if constexpr (V == V_LWWMAP || V == V_PNCMAP || V == V_ORMM || V == V_LWWMAP_DELTA)  // (single-rank engines only: no owner-mode instantiation)
    if (mode == M_OWNER) return hipErrorInvalidValue;
  switch (mode * 2 + (skew ? 1u : 0u)) {
    case M_FUSED * 2: hipLaunchKernelGGL((k_bucket_apply<W, M, true, false, false>), g, blk, 0, s, ba); break;
    case M_FUSED * 2 + 1: hipLaunchKernelGGL((k_bucket_apply<W, M, true, true, false>), g, blk, 0, s, ba); break;
    case M_OWNER * 2:
      if constexpr (V != V_LWWMAP && V != V_PNCMAP && V != V_ORMM && V != V_LWWMAP_DELTA) hipLaunchKernelGGL((k_bucket_apply<W, M, false, false, true>), g, blk, 0, s, ba);
      break;
    case M_OWNER * 2 + 1:
      if constexpr (V != V_LWWMAP && V != V_PNCMAP && V != V_ORMM && V != V_LWWMAP_DELTA) hipLaunchKernelGGL((k_bucket_apply<W, M, false, true, true>), g, blk, 0, s, ba);
      break;
    case M_BYPASS * 2: hipLaunchKernelGGL((k_bucket_apply<W, M, false, false, false>), g, blk, 0, s, ba); break;
    case M_BYPASS * 2 + 1: hipLaunchKernelGGL((k_bucket_apply<W, M, false, true, false>), g, blk, 0, s, ba); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the variants of this group, V in [0, V_N)
template <uint32_t V>
hipError_t group_dispatch(uint32_t vid, uint32_t mode, bool skew, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if constexpr (V >= V_N) {
    return hipErrorInvalidValue;
  } else {
    if constexpr (kVariantGroup[V] == AGX_VGROUP)
      if (vid == V) return launch_v<V>(mode, skew, g, s, ba);
    return group_dispatch<V + 1>(vid, mode, skew, g, s, ba);
  }
}

// a feature's fast launch of the plain variant V: k_bucket_apply<.., KM | F, .., kPrio> in the single-rank modes
template <uint32_t V, uint32_t F, bool kPrio>
hipError_t launch_feature(uint32_t mode, dim3 g, hipStream_t s, const BucketArgs& ba) {
  constexpr uint32_t M = kVariants[V].km | F;
  if (mode == M_FUSED)
    hipLaunchKernelGGL((k_bucket_apply<false, M, true, false, false, kPrio>), g, dim3(kBThreads), 0, s, ba);
  else if (mode == M_BYPASS)
    hipLaunchKernelGGL((k_bucket_apply<false, M, false, false, false, kPrio>), g, dim3(kBThreads), 0, s, ba);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// the feature launches of group G: kPrio of the catch-all plain variants, the KM flag combinations of the
// compiled catch-all variant (agx_launch_apply_feature)
template <uint32_t G>
hipError_t feature_dispatch(uint32_t vid, uint32_t mode, uint32_t km_flags, bool prio, dim3 g, hipStream_t s,
                            const BucketArgs& ba) {
  if (prio && km_flags) return hipErrorInvalidValue;
  if constexpr (kVariantGroup[V_ALL] == G)
    if (vid == V_ALL && prio) return launch_feature<V_ALL, 0, true>(mode, g, s, ba);
  if constexpr (kVariantGroup[V_ALL_COMPILED] == G) {
    static_assert(kVariantGroup[V_ALL_COMPILED] == G, "the flag combinations live in V_ALL_COMPILED's group");
    if (vid == V_ALL_COMPILED) {
      if (prio) return launch_feature<V_ALL_COMPILED, 0, true>(mode, g, s, ba);
      switch (km_flags) {
        case kStashKM: return launch_feature<V_ALL_COMPILED, kStashKM, false>(mode, g, s, ba);
        case kTimersKM: return launch_feature<V_ALL_COMPILED, kTimersKM, false>(mode, g, s, ba);
        case kTimersKM | kIdleKM: return launch_feature<V_ALL_COMPILED, kTimersKM | kIdleKM, false>(mode, g, s, ba);
        case kTimersKM | kIdleKM | kShardKM:
          return launch_feature<V_ALL_COMPILED, kTimersKM | kIdleKM | kShardKM, false>(mode, g, s, ba);
        case kTimersKM | kAskKM: return launch_feature<V_ALL_COMPILED, kTimersKM | kAskKM, false>(mode, g, s, ba);
        case kWatchKM: return launch_feature<V_ALL_COMPILED, kWatchKM, false>(mode, g, s, ba);
        case kWatchKM | kChildKM: return launch_feature<V_ALL_COMPILED, kWatchKM | kChildKM, false>(mode, g, s, ba);
        case kSuperKM: return launch_feature<V_ALL_COMPILED, kSuperKM, false>(mode, g, s, ba);
        case kRecepKM: return launch_feature<V_ALL_COMPILED, kRecepKM, false>(mode, g, s, ba);
        case kRecepKM | kHashKM: return launch_feature<V_ALL_COMPILED, kRecepKM | kHashKM, false>(mode, g, s, ba);
        case kRecepKM | kTopicKM: return launch_feature<V_ALL_COMPILED, kRecepKM | kTopicKM, false>(mode, g, s, ba);
        case kRecepKM | kTopicKM | kListKM:
          return launch_feature<V_ALL_COMPILED, kRecepKM | kTopicKM | kListKM, false>(mode, g, s, ba);
      }
    }
  }
  // restartWithBackoff: a unit of its own (kBackoffGroup), so that V_ALL_COMPILED's unit compiles what it compiled before
  if constexpr (G == kBackoffGroup)
    if (vid == V_ALL_COMPILED && !prio && km_flags == (kSuperKM | kBackoffKM))
      return launch_feature<V_ALL_COMPILED, kSuperKM | kBackoffKM, false>(mode, g, s, ba);
  return hipErrorInvalidValue;
}

// k_tiny_apply of the plain / compiled variants of this group
template <uint32_t V>
hipError_t tiny_dispatch(uint32_t vid, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if constexpr (V >= V_N) {
    return hipErrorInvalidValue;
  } else {
    if constexpr (kVariantGroup[V] == AGX_VGROUP && !kVariants[V].wide)
      if (vid == V) {
        hipLaunchKernelGGL((k_tiny_apply<kVariants[V].km>), g, dim3(kTinyThreads), 0, s, ba);
        return hipGetLastError();
      }
    return tiny_dispatch<V + 1>(vid, g, s, ba);
  }
}

// k_dense_apply / k_dense_fused of the plain / compiled variants of this group
template <uint32_t V>
hipError_t dense_dispatch(uint32_t vid, uint32_t mode, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if constexpr (V >= V_N) {
    return hipErrorInvalidValue;
  } else {
    if constexpr (kVariantGroup[V] == AGX_VGROUP && !kVariants[V].wide)
      if (vid == V) {
        if (mode == M_FUSED)
          hipLaunchKernelGGL((k_dense_fused<kVariants[V].km, false>), g, dim3(kDenseThreads), 0, s, ba);
        else if (mode == M_PERSIST)
          hipLaunchKernelGGL((k_dense_fused<kVariants[V].km, false, true>), g, dim3(kDenseThreads), 0, s, ba);
        else if (mode == M_OWNER)
          hipLaunchKernelGGL((k_dense_fused<kVariants[V].km, true>), g, dim3(kDenseThreads), 0, s, ba);
        else
          hipLaunchKernelGGL((k_dense_apply<kVariants[V].km>), g, dim3(kDenseThreads), 0, s, ba);
        return hipGetLastError();
      }
    return dense_dispatch<V + 1>(vid, mode, g, s, ba);
  }
}

template <uint32_t V>
hipError_t persist_occ(uint32_t vid, int* n) {
  if constexpr (V >= V_N) {
    return hipErrorInvalidValue;
  } else {
    if constexpr (kVariantGroup[V] == AGX_VGROUP && !kVariants[V].wide)
      if (vid == V)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(n, k_dense_fused<kVariants[V].km, false, true>,
                                                            kDenseThreads, 0);
    return persist_occ<V + 1>(vid, n);
  }
}

// k_ring_apply (tiny: k_ring_tiny) of the plain / compiled variants of this group
template <uint32_t V>
hipError_t ring_dispatch(uint32_t vid, bool tiny, dim3 g, hipStream_t s, const BucketArgs& ba, const RingArgs& ra) {
  if constexpr (V >= V_N) {
    return hipErrorInvalidValue;
  } else {
    if constexpr (kVariantGroup[V] == AGX_VGROUP && !kVariants[V].wide)
      if (vid == V) {
        if (tiny)
          hipLaunchKernelGGL((k_ring_tiny<kVariants[V].km>), g, dim3(kTinyThreads), 0, s, ba, ra);
        else
          hipLaunchKernelGGL((k_ring_apply<kVariants[V].km>), g, dim3(kBThreads), 0, s, ba, ra);
        return hipGetLastError();
      }
    return ring_dispatch<V + 1>(vid, tiny, g, s, ba, ra);
  }
}

}  // namespace

const GroupLaunch& AGX_CAT(agx_group_, AGX_VGROUP)() {
  static const GroupLaunch launch = {group_dispatch<0>, feature_dispatch<AGX_VGROUP>, tiny_dispatch<0>,
                                     dense_dispatch<0>, ring_dispatch<0>, persist_occ<0>};
  return launch;
}

#if AGX_VGROUP == 9
static_assert(kLwwmapGroup == 9, "k_lwwmap_merge lives in V_LWWMAP's unit");
hipError_t agx_launch_lwwmap_merge(dim3 g, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                   const uint32_t* orw_n, const uint32_t* step0, uint32_t slot, uint32_t clock, int64_t base) {
  hipLaunchKernelGGL(k_lwwmap_merge, g, dim3(kThreads), 0, s, P, orw, orm, orw_n, step0, slot, clock, (long long)base);
  return hipGetLastError();
}
#endif

#if AGX_VGROUP == 10
static_assert(kPncmapGroup == 10, "k_pncmap_merge lives in V_PNCMAP's unit");
hipError_t agx_launch_pncmap_merge(dim3 g, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                   const uint32_t* orw_n) {
  hipLaunchKernelGGL(k_pncmap_merge, g, dim3(kThreads), 0, s, P, orw, orm, orw_n);
  return hipGetLastError();
}
#endif

#if AGX_VGROUP == 11
static_assert(kOrmmGroup == 11, "k_ormm_merge lives in V_ORMM's unit");
hipError_t agx_launch_ormm_merge(dim3 g, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                 const uint32_t* orw_n) {
  hipLaunchKernelGGL(k_ormm_merge, g, dim3(kThreads), 0, s, P, orw, orm, orw_n);
  return hipGetLastError();
}
#endif

#if AGX_VGROUP == 12
static_assert(kLwwmapDeltaGroup == 12, "k_lwwmap_delta_merge lives in V_LWWMAP_DELTA's unit");
namespace {
// LWWMap populations with delta replication (agx_set_lwwmap_delta): the state effects of every replica run the
// apply listed (lwd_protocol did the tells, the row allocation and the placeholder decisions): one wave per
// replica, lane = key = ring slot (lwwmap_delta_merge_wave).  The clock arguments as k_lwwmap_merge's.  Defined here, not in
// agx_kernels.h: only this unit launches it, so only this unit compiles it.
__global__ void __launch_bounds__(kThreads) k_lwwmap_delta_merge(DevParams P, const uint4* orw, const uint2* orm,
                                                                    const uint32_t* orw_n, const uint32_t* step0,
                                                                    uint32_t slot, uint32_t clock, long long base) {
  const uint32_t n = orw_n[0];
  const CrdtHeap H = crdt_heap(P);
  const int64_t now = (int64_t)base + (int64_t)((uint64_t)*step0 + slot + 1ull);
  const uint32_t nw = gridDim.x * (kThreads / kWave);
  // the wave's index through readfirstlane: the compiler then knows the run, its messages and the replica's
  // version vector, deltaVersions and selector words to be wave-uniform (scalar registers, scalar branches)
  const uint32_t it0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave));
  for (uint32_t it = it0; it < n; it += nw) {
    const uint4 w = orw[it];
    const uint2* msg = orm + w.z;
    lwwmap_delta_merge_wave(P, H, w.x, w.y & 0xFFu, w.y >> 8, w.w, clock, now, [&](uint32_t q) { return msg[q].x; },
                            [&](uint32_t q) { return msg[q].y; });
  }
}
}  // namespace
hipError_t agx_launch_lwwmap_delta_merge(dim3 g, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                         const uint32_t* orw_n, const uint32_t* step0, uint32_t slot, uint32_t clock,
                                         int64_t base) {
  hipLaunchKernelGGL(k_lwwmap_delta_merge, g, dim3(kThreads), 0, s, P, orw, orm, orw_n, step0, slot, clock, (long long)base);
  return hipGetLastError();
}
#endif

#if AGX_VGROUP == 0
namespace {
#define AGX_GROUP_REF(g) agx_group_##g,
const GroupLaunch& (*const kGroups[kVGroups])() = {AGX_GROUPS(AGX_GROUP_REF)};
const GroupLaunch& group_of(uint32_t vid) { return kGroups[kVariantGroup[vid]](); }
}  // namespace

hipError_t agx_launch_apply(uint32_t vid, uint32_t mode, bool skew, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if (vid >= V_N) return hipErrorInvalidValue;
  return group_of(vid).apply(vid, mode, skew, g, s, ba);
}

hipError_t agx_launch_apply_feature(uint32_t vid, uint32_t mode, uint32_t km_flags, bool prio, dim3 g, hipStream_t s,
                                    const BucketArgs& ba) {
  if (vid >= V_N) return hipErrorInvalidValue;
  if (km_flags == (kSuperKM | kBackoffKM)) return kGroups[kBackoffGroup]().feature(vid, mode, km_flags, prio, g, s, ba);
  return group_of(vid).feature(vid, mode, km_flags, prio, g, s, ba);
}

hipError_t agx_launch_ring(uint32_t vid, bool tiny, dim3 g, hipStream_t s, const BucketArgs& ba, const RingArgs& ra) {
  if (vid >= V_N || kVariants[vid].wide) return hipErrorInvalidValue;
  return group_of(vid).ring(vid, tiny, g, s, ba, ra);
}

hipError_t agx_launch_dense(uint32_t vid, uint32_t mode, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if (vid >= V_N || kVariants[vid].wide) return hipErrorInvalidValue;
  return group_of(vid).dense(vid, mode, g, s, ba);
}

hipError_t agx_dense_persist_occupancy(uint32_t vid, int* n) {
  *n = 0;
  if (vid >= V_N || kVariants[vid].wide) return hipErrorInvalidValue;
  return group_of(vid).persist_occupancy(vid, n);
}

hipError_t agx_launch_tiny(uint32_t vid, dim3 g, hipStream_t s, const BucketArgs& ba) {
  if (vid >= V_N || kVariants[vid].wide) return hipErrorInvalidValue;
  return group_of(vid).tiny(vid, g, s, ba);
}
#endif

}  // namespace agx
