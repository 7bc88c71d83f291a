// agx_variants.h — the k_bucket_apply instantiations the engine launches, and where they live.
//
// Every (behaviour-mask variant, pipeline mode, fast/skew) combination is a separate kernel
// (k_bucket_apply<kWide, KM, kGather, kSkew, kOwner>, agx_kernels.h).  They are instantiated in
// agx_apply.hip, which the build compiles once per variant group (-DAGX_VGROUP=g), so the ~100
// kernels compile in parallel translation units instead of one; the host runtime
// (agx_engine.hip) only calls agx_launch_apply().
#pragma once
#include "agx_kernels.h"

namespace agx {

struct ApplyVariant {
  bool wide;    // CRDT state gossips (snapshot heap) possible
  uint32_t km;  // behaviour-kind mask the variant is specialised to
};

constexpr uint32_t kCrdtKM = kb(AGX_KIND_GCOUNTER) | kb(AGX_KIND_PNCOUNTER) | kb(AGX_KIND_ORSET);

// variant ids (the engine picks one from the registered kinds, agx_engine.hip launch_apply)
enum : uint32_t {
  V_GC_DELTA = 0, V_PN_DELTA, V_OR_DELTA, V_ALL_DELTA,
  V_GC, V_PN, V_OR, V_CRDT, V_ALL_WIDE,
  V_RING, V_FWD, V_FANOUT, V_COUNTER, V_COMPILED, V_ALL_COMPILED, V_ALL,
  V_LWWMAP,  // LWWMap replicas only (agx_lwwmap.h); appended: the ids above do not move
  V_PNCMAP,  // PNCounterMap replicas only (agx_pncmap.h); appended likewise
  V_ORMM,    // ORMultiMap replicas only (agx_ormm.h); appended likewise
  V_LWWMAP_DELTA,  // LWWMap replicas with delta replication (agx_lwwmap_delta.h); appended likewise
  V_N
};
constexpr ApplyVariant kVariants[V_N] = {
    {true, kb(AGX_KIND_GCOUNTER) | kDeltaKM}, {true, kb(AGX_KIND_PNCOUNTER) | kDeltaKM},
    {true, kb(AGX_KIND_ORSET) | kDeltaKM},    {true, KM_ALL | kDeltaKM},
    {true, kb(AGX_KIND_GCOUNTER)},            {true, kb(AGX_KIND_PNCOUNTER)},
    {true, kb(AGX_KIND_ORSET)},               {true, kCrdtKM},
    {true, KM_ALL},                           {false, kb(AGX_KIND_RING)},
    {false, kb(AGX_KIND_FORWARD_RR)},         {false, kb(AGX_KIND_FANOUT)},
    {false, kb(AGX_KIND_COUNTER)},            {false, kb(AGX_KIND_COMPILED)},
    {false, KM_ALL | kb(AGX_KIND_COMPILED)},  {false, KM_ALL},
    {true, kb(AGX_KIND_LWWMAP)},
    {true, kb(AGX_KIND_PNCOUNTERMAP)},
    {true, kb(AGX_KIND_ORMULTIMAP)},
    {true, kb(AGX_KIND_LWWMAP) | kDeltaKM},
};
static_assert((kb(AGX_KIND_LWWMAP) & (KM_ALL | kCrdtKM | kb(AGX_KIND_COMPILED))) == 0 && kb(AGX_KIND_LWWMAP) < kBackoffKM,
              "the LWWMap kind has a mask bit of its own");
static_assert((kb(AGX_KIND_PNCOUNTERMAP) & (KM_ALL | kCrdtKM | kb(AGX_KIND_COMPILED) | kb(AGX_KIND_LWWMAP))) == 0 &&
                  kb(AGX_KIND_PNCOUNTERMAP) < kBackoffKM,
              "the PNCounterMap kind has a mask bit of its own");
static_assert((kb(AGX_KIND_ORMULTIMAP) & (KM_ALL | kCrdtKM | kb(AGX_KIND_COMPILED) | kb(AGX_KIND_LWWMAP) |
                                          kb(AGX_KIND_PNCOUNTERMAP))) == 0 &&
                  kb(AGX_KIND_ORMULTIMAP) < kBackoffKM,
              "the ORMultiMap kind has a mask bit of its own");

// pipeline modes: fused single-rank gather (kGather), multi-rank owner grouping (kOwner),
// single-rank multi-pass with the backlog in place (neither)
enum : uint32_t { M_FUSED = 0, M_OWNER = 1, M_BYPASS = 2, M_PERSIST = 3 /* dense launch only: k_dense_fused<.., true> */ };

// variant groups = translation units (agx_apply.hip built with -DAGX_VGROUP=0..kVGroups-1);
// the heavy CRDT variants are spread so the units take similar time
constexpr uint32_t kVGroups = 13;
// the last group holds no variant of the table: it is the unit of the kSuperKM | kBackoffKM feature launches alone
constexpr uint32_t kBackoffGroup = 8;
// V_LWWMAP and k_lwwmap_merge are a unit of their own too, so that every other unit compiles what it compiled before
constexpr uint32_t kLwwmapGroup = 9;
// and so are V_PNCMAP and k_pncmap_merge
constexpr uint32_t kPncmapGroup = 10;
// and V_ORMM and k_ormm_merge
constexpr uint32_t kOrmmGroup = 11;
// and V_LWWMAP_DELTA and k_lwwmap_delta_merge
constexpr uint32_t kLwwmapDeltaGroup = 12;
constexpr uint32_t kVariantGroup[V_N] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7, kLwwmapGroup, kPncmapGroup, kOrmmGroup,
                                         kLwwmapDeltaGroup};

// launch k_bucket_apply<variant vid, mode, skew> with `grid` x kBThreads threads on `s`
// (defined in agx_apply.hip; returns hipErrorInvalidValue for an unknown combination)
hipError_t agx_launch_apply(uint32_t vid, uint32_t mode, bool skew, dim3 grid, hipStream_t s, const BucketArgs& ba);
// launch a feature's fast launch k_bucket_apply<variant vid, mode, no skew, KM | km_flags, kPrio = prio> (agx_engine.hip
// kFeatures: km_flags = the feature's KM flag bits, or none and `prio` for priority mailboxes).  Instantiated in the
// modes M_FUSED / M_BYPASS: kPrio for the catch-all plain variants V_ALL / V_ALL_COMPILED, the flag combinations
// kStashKM, kTimersKM, kTimersKM | kIdleKM, kTimersKM | kIdleKM | kShardKM, kTimersKM | kAskKM, kWatchKM, kWatchKM | kChildKM, kSuperKM, kRecepKM,
// kRecepKM | kHashKM, kRecepKM | kTopicKM, kRecepKM | kTopicKM | kListKM for V_ALL_COMPILED, all in
// V_ALL_COMPILED's group, and kSuperKM | kBackoffKM for V_ALL_COMPILED in kBackoffGroup
// (hipErrorInvalidValue otherwise)
hipError_t agx_launch_apply_feature(uint32_t vid, uint32_t mode, uint32_t km_flags, bool prio, dim3 grid, hipStream_t s,
                                    const BucketArgs& ba);
// launch k_lwwmap_merge after V_LWWMAP's apply (defined in kLwwmapGroup's unit): the runs the apply listed in
// orw / orm / orw_n; the clock's logical time is base + *step0 + slot + 1 (agx_kernels.h)
hipError_t agx_launch_lwwmap_merge(dim3 grid, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                   const uint32_t* orw_n, const uint32_t* step0, uint32_t slot, uint32_t clock, int64_t base);
// launch k_lwwmap_delta_merge after V_LWWMAP_DELTA's apply (defined in kLwwmapDeltaGroup's unit): the arguments of
// agx_launch_lwwmap_merge
hipError_t agx_launch_lwwmap_delta_merge(dim3 grid, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                         const uint32_t* orw_n, const uint32_t* step0, uint32_t slot, uint32_t clock,
                                         int64_t base);
// launch k_pncmap_merge after V_PNCMAP's apply (defined in kPncmapGroup's unit): the runs the apply listed in
// orw / orm / orw_n
hipError_t agx_launch_pncmap_merge(dim3 grid, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                   const uint32_t* orw_n);
// launch k_ormm_merge after V_ORMM's apply (defined in kOrmmGroup's unit): the runs the apply listed in
// orw / orm / orw_n
hipError_t agx_launch_ormm_merge(dim3 grid, hipStream_t s, const DevParams& P, const uint4* orw, const uint2* orm,
                                 const uint32_t* orw_n);
// launch k_tiny_apply<variant vid's kinds> (plain / compiled variants only: hipErrorInvalidValue otherwise)
hipError_t agx_launch_tiny(uint32_t vid, dim3 grid, hipStream_t s, const BucketArgs& ba);
// launch k_dense_apply<variant vid's kinds> (mode M_FUSED / M_OWNER: k_dense_fused) (plain / compiled variants only)
hipError_t agx_launch_dense(uint32_t vid, uint32_t mode, dim3 grid, hipStream_t s, const BucketArgs& ba);
// resident blocks per CU of the persistent fused dense launch of variant vid (0: not a dense variant)
hipError_t agx_dense_persist_occupancy(uint32_t vid, int* blocks_per_cu);
// launch k_ring_apply<variant vid's kinds> (tiny: k_ring_tiny, kTinyThreads) (plain / compiled variants only)
hipError_t agx_launch_ring(uint32_t vid, bool tiny, dim3 grid, hipStream_t s, const BucketArgs& ba, const RingArgs& ra);

}  // namespace agx
