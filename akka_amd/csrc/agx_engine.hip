// agx_engine.hip — host runtime of the MI355X batched actor-dispatch engine
// and the C ABI declared in include/akka_gpu.h.
//
// One engine = one rank = one GPU (or one virtual rank of a loopback group).
// Actor state and envelopes live structure-of-arrays in HBM; a superstep is
//   [exchange (R > 1)] -> compaction -> stable radix sort by destination ->
//   segmented drain + behaviour-apply (emits the next step's tells).
// No host round trip per superstep on one GPU; with R > 1 the host reads the
// per-peer counts once per superstep to size the RCCL send/recv group.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "agx_kernels.h"
#include "agx_tellq.h"
#include "agx_variants.h"

using namespace agx;

namespace {

thread_local std::string g_err;

agx_status set_err(agx_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return st;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return set_err(AGX_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                     __LINE__);                                                                \
  } while (0)

#define NCCL_TRY(expr)                                                                            \
  do {                                                                                            \
    ncclResult_t _r = (expr);                                                                     \
    if (_r != ncclSuccess)                                                                        \
      return set_err(AGX_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(_r), __FILE__, \
                     __LINE__);                                                                   \
  } while (0)

#define AGX_TRY(expr)              \
  do {                             \
    agx_status _s = (expr);        \
    if (_s != AGX_OK) return _s;   \
  } while (0)

uint32_t ceil_log2(uint64_t x) {
  uint32_t b = 0;
  while ((1ull << b) < x) ++b;
  return b;
}

int32_t java_hash_decimal(uint32_t id) {
  char buf[16];
  int n = 0;
  do {
    buf[n++] = (char)('0' + id % 10u);
    id /= 10u;
  } while (id);
  uint32_t h = 0;
  for (int i = n - 1; i >= 0; --i) h = h * 31u + (uint32_t)buf[i];
  return (int32_t)h;
}

struct DevMsgs {
  uint32_t* key = nullptr;
  uint32_t* src = nullptr;
  uint32_t* pay = nullptr;
  Msgs m() const { return {key, src, pay}; }
  CMsgs c() const { return {key, src, pay}; }
};

enum KClass { K_CROWSCAN, K_CDOWN, K_UPSWEEP, K_ROWSCAN, K_DOWNSWEEP, K_APPLY, K_EXCHANGE, K_MCOMPACT, K_SKEW, K_TICK,
              K_BOUNDS, K_SKEWPRE, K_TINY, K_RINGAPPLY, K_DENSE, K_NCLASS };
const char* kClassNames[K_NCLASS] = {"chunk_rowscan", "chunk_downsweep", "sort_upsweep", "sort_rowscan",
                                     "sort_downsweep", "bucket_apply", "exchange", "mcompact", "bucket_apply_skew",
                                     "fused_tick", "bucket_bounds", "skew_prepass", "bucket_apply_tiny",
                                     "ring_apply", "bucket_apply_dense"};

constexpr uint32_t kGraphSizes[5] = {1, 2, 4, 8, 16};  // superstep replays (agx_engine::gx)
constexpr uint32_t kRowAlign = 32;  // CRDT row pitch (u32) of rows wider than one 128-B line
constexpr uint32_t kStatBlk = 16;                    // d_stats block (see agx_engine::d_stats)
constexpr uint32_t kStatSred = ST_N, kStatInfl = ST_N + kBStats;
static_assert(kStatInfl < kStatBlk, "stats block layout");

struct SortPlan {  // LSD passes over key bits [bb, key_bits)
  uint32_t npass = 1;
  uint32_t shift[4] = {0}, bits[4] = {0};
};

}  // namespace

struct agx_engine {
  agx_cfg cfg{};
  TellQueue tq;  // agx_tell: the lock-free tell path (agx_tellq.h), taken by agx_run
  hipStream_t stream = nullptr;
  uint64_t n_global = 0, n_local = 0, cap = 0, cap_emit = 0;
  uint32_t max_supers = 1, dstride = 4, dsub = kSub;  // dense passes: super-tiles (at most), table row stride, max tiles
                                                      // per super-tile (the size itself is chosen per pass: pass_super)
  uint32_t T = 1, C = 0, W = 1, kmax = 1, R = 1, rank = 0, num_shards = 1000, key_bits = 1;
  uint32_t Traw = 1;  // dispatcher throughput (>= 1); T = min(Traw, C) for the default mailbox class
  // mailbox classes (agx_set_mailbox_class): capacity per class, class 0 = cfg.capacity
  uint32_t mcap[AGX_MAX_MAILBOX_CLASSES] = {0};
  uint32_t mclass_set = 1u;  // bit c: class c configured (class 0 always)
  bool mclasses = false;     // some class other than 0 configured: kernels look up per-actor limits
  // priority tables (agx_set_mailbox_priority): bit c of prio_mask = class c has one.  An engine with a
  // table launches the prioritised catch-all variants (apply_variant, launch_apply) and no wave / ring /
  // dense / persistent launch
  uint32_t prio_mask = 0;
  std::vector<uint8_t> prio_tab = std::vector<uint8_t>(AGX_MAX_MAILBOX_CLASSES * 256u, 0);
  uint8_t* d_ptab = nullptr;  // [classes][256] tables, then the [nb] bucket marks (DevParams.ptab)
  bool prio_dirty = false;   // the tables or the actors' classes changed since the last upload
  // deque-based mailboxes (agx_set_stash): the classes' stash capacities.  An engine with one launches the
  // stash instantiation of the compiled catch-all variant and no wave / ring / dense / persistent launch
  uint32_t stash_cap[AGX_MAX_MAILBOX_CLASSES] = {0};
  bool stash_on = false;
  uint32_t* d_stash = nullptr;  // DevParams.stash (agx_device.h StashDev): sized at the first run
  uint32_t stash_smax = 0, stash_pmax = 0;
  size_t stash_hdr_off = 0, stash_slot_off = 0;  // u32 offsets of the headers / envelopes in d_stash
  bool stash_dirty = false;  // the capacities or the actors' classes changed since the last upload
  bool beh_stash = false;    // the compiled tables hold a stash / unstash_all result (agx_set_behaviors)
  // timers (agx_set_timers): n_keys slots per actor.  An engine with timers launches the timer instantiation of
  // the compiled catch-all variant and no wave / ring / dense / persistent launch
  uint32_t tm_keys = 0;
  uint32_t* d_timers = nullptr;  // DevParams.timers (agx_device.h TimerDev): sized at the first run
  uint32_t beh_tm_keys = 0;      // the compiled tables use timer keys below this (0: no timer action / AGX_V_TIMER)
  bool tm_bad_start = false;     // agx_start_timers was called on an engine without timers: agx_run refuses
  uint64_t tm_ticks = 0;         // supersteps that ran while the engine was not quiescent
  uint32_t tm_clock = 0;         // the device clock after the last run (every bucket's tick count)
  struct TimerStart {
    uint64_t first, count;
    uint32_t key, periodic, delay, payload;
    std::vector<uint32_t> delays;
  };
  std::vector<TimerStart> tm_starts;  // agx_start_timers calls not yet applied on the device (prepare_run)
  // receive timeouts (agx_set_receive_timeout), on top of the timers: three [actor] rows and the transparent-tag
  // mask appended to the timer storage.  Such an engine launches the kTimers | kIdle instantiation
  bool rt_on = false;
  uint32_t rt_mask[8] = {0};   // bit t: messages of tag t are NotInfluenceReceiveTimeout
  bool beh_rt = false;         // the compiled tables set or cancel a receive timeout
  bool beh_rt_tag = false;     // the compiled tables name tag 0xFB (an or_mask or a tag test)
  bool rt_bad_start = false;   // agx_start_receive_timeout was called on an engine without the feature: agx_run refuses
  struct RtStart {
    uint64_t first, count;
    uint32_t delay, payload;
  };
  std::vector<RtStart> rt_starts;  // agx_start_receive_timeout calls not yet applied on the device (prepare_run)
  // sharded entities (agx_set_sharding), on top of receive timeouts: the entity types and the storage (agx_device.h
  // ShardDev), whose address stands in the timer storage
  std::vector<agx_entity_type> sh_types;
  uint32_t* d_shard = nullptr;
  bool beh_passivate = false;  // the compiled tables hold AGX_A_PASSIVATE
  // the ask pattern (agx_set_ask), on top of the timers: one [key][actor] row appended to the timer storage.  Such an
  // engine launches the kTimers | kAsk instantiation
  bool ask_on = false;
  uint32_t beh_ask_keys = 0;      // the compiled tables hold ask actions on keys below this (0: none)
  int64_t beh_ask_unpaired = -1;  // the first AGX_A_ASK_SEND not directly preceded by the ARM of its key, or ARM without its SEND
  // death watch (agx_set_death_watch): n_slots watch slots per actor.  Such an engine launches the watch
  // instantiation of the compiled catch-all variant and no wave / ring / dense / persistent launch
  uint32_t wd_slots = 0;
  uint32_t* d_watch = nullptr;  // DevParams.watch (agx_device.h WatchDev)
  bool beh_watch = false;       // the compiled tables hold a watch action or a signal case
  bool wd_bad_start = false;    // agx_start_watch was called on an engine without death watch: agx_run refuses
  bool wd_died_init = false;    // the death ticks follow the registered actors (before the first run)
  uint64_t wd_ticks = 0;        // supersteps that ran while the engine was active
  uint32_t wd_clock = 0;        // the device clock after the last run (every bucket's tick count)
  struct WatchStart {
    uint64_t first, count;
    int64_t offset;
    uint32_t with, payload;
    std::vector<uint32_t> watchees;
  };
  std::vector<WatchStart> wd_starts;  // agx_start_watch calls not yet applied on the device (prepare_run)
  // children (agx_set_children): regions and spawn sites on an engine with death watch.  Such an engine launches
  // the children instantiation of the compiled catch-all variant (kWatch | kChild)
  std::vector<agx_child_region> ch_regions;
  std::vector<agx_spawn_site> ch_sites;
  uint32_t* d_child = nullptr;  // the child storage (agx_device.h ChildDev); its address stands in the watch storage
  bool beh_child = false;       // the compiled tables spawn, stop a child or read AGX_V_SPAWNED / AGX_V_CHILD
  bool beh_ctl_tags = false;    // the compiled tables name tag 0xFD or 0xFC (an or_mask or a tag test)
  bool ch_bad_spawn = false;    // agx_spawn_children was called on an engine without children: agx_run refuses
  struct ChildSpawn {
    uint64_t first, count;
    uint32_t site, arg;
  };
  std::vector<ChildSpawn> ch_spawns;  // agx_spawn_children calls not yet applied on the device (prepare_run)
  // supervision (agx_set_supervision): strategy entries per compiled behaviour.  Such an engine launches the
  // supervision instantiation of the compiled catch-all variant and no wave / ring / dense / persistent launch
  bool sv_on = false;
  uint32_t sv_levels = 0, sv_beh = 0;
  uint32_t* d_super = nullptr;         // DevParams.super (agx_device.h SuperDev)
  std::vector<agx_supervisor> sv_tab;  // [behaviour][AGX_MAX_SUPERVISORS], as on the device
  std::vector<uint8_t> h_init;         // the kind every actor was registered with (empty without supervision)
  bool sv_init_dirty = false;          // h_init is newer than the device's copy
  bool beh_fail = false;               // the compiled tables hold an AGX_RES_FAIL case
  bool beh_svsig = false;              // ... a PreRestart / PostStop signal case
  bool beh_vstash = false;             // ... an AGX_V_STASH operand
  uint32_t beh_sv_tells = 0;           // the most tells a failing or stopping case and a supervision signal case of one behaviour make together
  uint64_t sv_ticks = 0;               // supersteps with mail so far (= agx_stats.supersteps)
  uint32_t sv_clock = 0;               // the device clock after the last run (every bucket's launch count)
  // restartWithBackoff (agx_set_backoff), on top of supervision: such an engine launches the backoff instantiation
  uint32_t* d_backoff = nullptr;       // agx_device.h BackoffDev (its address stands in d_super's header)
  std::vector<agx_backoff> bo_tab;     // [behaviour][AGX_MAX_SUPERVISORS]
  std::vector<agx_supervisor> bo_sv;   // the supervision table the rows were checked against (sv_tab then)
  uint32_t bo_levels = 0, bo_beh = 0;
  // the receptionist (agx_set_receptionist): service keys, per-actor key masks, listings.  Such an engine launches
  // the receptionist instantiation of the compiled catch-all variant, then the rebuild kernels, every superstep
  uint32_t* d_recep = nullptr;   // DevParams.recep (agx_device.h RecepDev)
  uint32_t rc_keys = 0, rc_cap = 0;
  uint32_t beh_rc_keys = 0;      // the service keys the compiled tables use (the largest index + 1)
  bool beh_recep = false;        // the compiled tables register, deregister, route, forward or read a listing
  bool rc_bad_start = false;     // agx_register_services was called on an engine without the receptionist: agx_run refuses
  struct RecepStart {
    uint64_t first, count;
    uint32_t key, on;
  };
  std::vector<RecepStart> rc_starts;  // agx_register_services calls not yet applied on the device
  // pub-sub topics (agx_set_topics), on top of the receptionist: the publication log, the per-bucket due counts.
  // Such an engine launches the kRecep | kTopic instantiation, then k_topic_plan beside the rebuild kernels
  uint32_t* d_topic = nullptr;   // (its address stands in the receptionist's storage: agx_device.h TopicDev)
  uint32_t tp_cap = 0;           // log_capacity
  bool beh_publish = false;      // the compiled tables publish
  struct TopicPub { uint32_t key, sender, payload; };
  std::vector<TopicPub> tp_pubs;  // agx_publish calls not yet applied on the device
  // Subscribe / Listing (agx_set_listings), on top of topics: the sub and pending masks, the per-bucket counts and due
  // words.  Such an engine launches the kRecep | kTopic | kList instantiation, then k_listing_plan after k_topic_plan
  uint32_t* d_list = nullptr;    // (its address stands in the receptionist's storage: agx_device.h ListDev)
  bool beh_listing = false;      // the compiled tables subscribe to or find a listing
  struct ListStart {
    uint64_t first, count;
    uint32_t key, on;
  };
  std::vector<ListStart> ls_starts;  // agx_subscribe_listings calls not yet applied on the device
  // consistent-hashing and random routing (agx_set_router_logics), on top of the receptionist: the hash rings.  Such
  // an engine launches the kRecep | kHash instantiation, and the ring kernels after the rebuild kernels
  uint32_t* d_hash = nullptr;    // (its address stands in the receptionist's storage: agx_device.h HashDev)
  uint32_t hr_mask = 0, hr_factor = 0, hr_npts = 0, hr_nseg = 0;
  bool beh_router = false;       // the compiled tables route by consistent hashing or at random
  uint32_t beh_hashed_keys = 0;  // the keys they route through by consistent hashing (a mask)
  int64_t beh_route_two = -1;    // the first action with two of BY_INDEX / HASHED / RANDOM (-1: none)
  // the reply path (agx_set_outbound): host-side actor ids and the outbox
  uint32_t host_lo = 0, host_n = 0;
  uint64_t outbox_cap = 0;
  uint32_t *d_outbox = nullptr, *d_outbox_n = nullptr;
  std::vector<uint32_t> outq;  // taken from the device, not yet handed to the host (dst, src, payload)
  uint64_t outbox_lost = 0;    // outbound tells dropped at a full outbox, not reported yet (agx_take_outbound)
  uint32_t bb = kBucketBits;  // bucket bits (agx_cfg.bucket_actors)

  // sharding tables (R > 1)
  std::vector<uint32_t> h_gid, h_route;
  // host mirrors of the actor SoA (uploaded before the first run after a change)
  std::vector<uint8_t> h_kind, h_alive;
  std::vector<uint64_t> h_state;  // word-major
  bool actors_dirty = true;
  uint32_t kinds_mask = 0;  // bit k set when some local actor has behaviour kind k (selects the apply variant)
  std::vector<uint64_t> h_row;  // local CSR rows (graph)
  std::vector<uint32_t> h_col;
  bool graph_set = false;

  uint8_t *d_kind = nullptr, *d_alive = nullptr;
  uint32_t *d_stopq = nullptr, *d_nstop = nullptr;
  uint64_t* d_state = nullptr;
  // CRDT engines (pw > 0 at the first upload) keep the device state actor-major, `pitch` u64 per
  // actor (a replica's words are one contiguous, 128-B aligned row); the host mirror stays word-major
  uint32_t pitch = 0;
  uint32_t *d_gid = nullptr, *d_route = nullptr;
  uint32_t ring_stride = 1, fan_k = 0;
  uint64_t fan_seed = 0, zipf_n = 0;
  uint32_t *d_zcdf = nullptr, *d_zperm = nullptr;
  uint2* d_zent = nullptr;
  uint64_t* d_row = nullptr;
  uint32_t* d_col = nullptr;
  // CRDT state gossips (agx_crdt.h): snapshot heap, 2 x cap rows of pw u32
  uint32_t pw = 0, gossip_f = 0;
  uint32_t delta_max = 0;  // delta-CRDT mode (agx_set_delta_crdt): Replicator max-delta-size, 0 = off
  bool layout_checked = false;  // RCCL: rows / tells sized alike on every rank (run_multi_rccl)
  uint32_t tiny_max = kTinyMax;  // multi-pass: inboxes up to this size take the wave path (AGX_TINY, 0 = off)
  // compiled behaviours (agx_set_behaviors)
  agx_case* d_bcase = nullptr;
  agx_act* d_bact = nullptr;
  uint32_t* d_bfirst = nullptr;
  uint32_t n_beh = 0;
  uint64_t heap_rows = 0;  // per parity: one region of 2^bb rows per bucket, then an overflow area of `cap` rows
  uint64_t gossip_seed = 0;
  uint32_t *d_heap = nullptr, *d_heap_top = nullptr, *d_step = nullptr;
  uint32_t *d_rx = nullptr, *d_s2rows = nullptr;  // multi-rank: received rows / rows packed for sending
  uint64_t rx_rows = 0;                            // rows of d_rx (>= cap; >= R x slab on the device path)
  uint32_t* d_srows = nullptr;                     // device-resident exchange: [R][slab][pw] row send slabs
  uint32_t *d_s2p = nullptr, *d_rcvp = nullptr;    // multi-rank: tells as (key, src, payload) triples, sent / received
  // device-resident multi-rank replays (run_multi_rccl, plain behaviours): fixed per-peer slabs of
  // `slab` envelopes, the replay's stop word halt[2] (k_mr_pack); h_halt = its pinned copy
  uint32_t *d_sslab = nullptr, *d_rslab = nullptr, *d_halt = nullptr, *h_halt = nullptr;
  uint32_t slab = 0;
  uint64_t mr_exact = 0;  // supersteps whose exchange the host redid exactly (a count over the slab)
  uint64_t mr_replays = 0;  // multi-rank replays launched as a captured graph
  // exchange accounting (agx_exchange_info): supersteps on the device-resident / host-planned
  // exchange, bytes this rank sent to its peers (envelopes + CRDT rows), and mr_host = 1 once every
  // rank agreed that the CRDT row slabs do not fit (mr_slabs) -- the host-planned path from then on
  uint64_t mr_dev_steps = 0, mr_host_steps = 0, mr_sent_env = 0, mr_sent_rows = 0;
  bool mr_host = false;
  bool mr_direct = false;  // the last device-resident superstep wrote its peer runs straight into the send slabs

  DevMsgs A, B, scr, bl, em, stg, s2;
  // single-rank multi-pass: the tell arena by superstep parity (em = even, em2 = odd superstep
  // counter): the apply writes one while identity grouping reads the other in place
  DevMsgs em2;
  bool ident_on = false;        // identity grouping enabled (multi-pass, > 1 radix pass; AGX_NO_IDENT=1 disables)
  uint4* d_emmeta = nullptr;    // [nb] per tell chunk: first key, last key, descents, descent position
  uint32_t *d_slsum = nullptr, *d_ident = nullptr;  // slice summaries; {on, rotation, total}
  uint64_t stg_cap = 0;
  uint32_t nb = 1, nchunks = 3;                // buckets; chunks = 2 nb + kStagedChunks
  uint32_t G = 1, ng = 1, nunits = 3, cstride = 4;  // first-pass histogram units (G buckets each)
  SortPlan plan;
  uint32_t *d_chunk_off = nullptr, *d_chunk_cnt = nullptr;
  uint32_t* d_hist_c = nullptr;  // [kRadix][cstride] first-pass histograms per unit
  uint32_t* d_hist_d = nullptr;  // [kRadix][dstride] dense-pass histograms per super-tile
  uint32_t *d_tot = nullptr, *d_bstart = nullptr, *d_n = nullptr, *d_total = nullptr, *d_moff0 = nullptr, *d_moff1 = nullptr;
  unsigned long long *d_bstats = nullptr, *d_sred = nullptr;  // per-block apply counters, their sum
  // d_stats = one block of kStatBlk u64: [0, ST_N) counters, [ST_N, +kBStats) = d_sred (sum of the
  // per-block apply counters), [kStatInfl] = d_inflight -- read back with ONE copy + ONE sync
  uint64_t *d_stats = nullptr, *d_cvec = nullptr, *d_cmat = nullptr, *d_inflight = nullptr;
  uint64_t* h_stat = nullptr;    // pinned copy of the d_stats block
  uint32_t* h_pin = nullptr;     // pinned ring of per-step totals
  uint64_t* h_pin64 = nullptr;   // pinned scratch (count matrix, stats)

  // fused superstep (single rank, one radix pass): gather-apply, parity-double-buffered arenas
  bool fused = false;
  DevMsgs bl2, eg0, eg1;
  uint32_t *d_tcnt[2] = {nullptr, nullptr}, *d_toff[2] = {nullptr, nullptr};
  uint32_t *d_blpre = nullptr, *d_ninbox = nullptr;  // multi-pass: backlog prefix, inbox total
  uint32_t *d_blo[2] = {nullptr, nullptr}, *d_blc[2] = {nullptr, nullptr}, *d_emc[2] = {nullptr, nullptr};
  uint32_t *d_stg_off = nullptr, *d_stg_cnt = nullptr, *d_ovf = nullptr, *d_cntb = nullptr, *d_parv = nullptr;
  uint32_t* h_cntb = nullptr;  // pinned [kLag][kGraphSteps][nb]: per-superstep inbox sizes of the replays in flight
  uint32_t cur_slot = 0;       // superstep index within the replay being captured / launched
  uint64_t host_steps = 0;     // fused: supersteps with mail, counted on the host from h_cntb
  uint32_t par = 0;  // fused: parity of the next superstep (host-tracked; graphs are captured per parity)
  uint32_t *d_skew_list = nullptr, *d_skew_n = nullptr;  // buckets for the general-path launch
  // single-rank multi-pass, plain behaviours: k_tiny_apply drains the buckets of <= tiny_max messages
  // one wave each and marks the others here ([nb]) for the block launch (AGX_TINY_LAUNCH=0: no wave
  // path, the block launch takes every bucket)
  uint32_t* d_blist = nullptr;
  uint32_t* d_dense_left = nullptr;  // [2] BucketArgs::dense_left
  bool tiny_launch = true;
  hipEvent_t tev[2] = {nullptr, nullptr};  // agx_run_timed: device time of a run (engine stream)
  bool timing = false;
  bool dense_fused = true;  // the dense launch also in the fused superstep (AGX_DENSE_FUSED=0: not)
  // the dense launch in the multi-rank (owner-grouping) superstep (AGX_DENSE_OWNER=0: not).  Round 6:
  // owner classes placed straight from registers (no staged multisplit) and the dense_left shortcut
  // (the block launch returns at entry when it took every bucket): R = 8 x 1M loopback, one hardware
  // queue, apply 32.7 us (block launch) -> 19.9 + 5.6 us (dense + returning block launch) per rank-step
  bool dense_owner = true;
  bool dense_alone = true;  // fused strict replays: the dense launch alone (cleared at its first recovery)
  bool recover_dense = false;  // run_single's recovery of a dense-alone superstep: the block + skew launches
  int dense_launch = -1;  // k_dense_apply before the block launch: 1 on, 0 off, -1 (default) ring populations
  // ring apply (agx_ring.h): bounded mailboxes whose queued messages stay in per-actor rings; decided
  // at the first run (setup_ring_apply), then k_ring_tiny + k_ring_apply per superstep replace the tiny /
  // block / skew launches.  On by default for deep bounded mailboxes (capacity >= kRingAutoC);
  // AGX_RING_APPLY=1 / 0 forces it.
  bool rg_on = false;
  uint32_t rg_c = 0, rg_dstride = 0;
  uint32_t *d_rg_state = nullptr, *d_rg_src = nullptr, *d_rg_pay = nullptr;
  uint32_t *d_rg_dk = nullptr, *d_rg_ds = nullptr, *d_rg_dp = nullptr;
  uint32_t* d_rg_nz = nullptr;  // [nb][64] non-empty-ring bits
  uint64_t em_cap = 0;  // entries of the tell arenas em / em2
  // multi-pass, plain behaviours: skewed buckets split over workgroups (k_skew_*, agx_kernels.h)
  uint32_t *d_sk_rec = nullptr, *d_sk_act = nullptr, *d_sk_pc = nullptr, *d_sk_meta = nullptr;
  uint32_t sk_budget = 0, sk_rows = 0;
  // bounded-mailbox rings (multi-pass, plain behaviours, every mailbox class bounded by <= kRingMaxC):
  // a skewed bucket's queued messages stay in per-actor rings instead of the backlog arena.
  // ring_res: pool slots whose drain scratch / tell slices were reserved after the arenas at
  // create (ring_lo0 = acap); the pool itself is allocated at the first run whose mailbox classes
  // allow it, with ring_c = the largest capacity, and fixes the classes from then on.
  uint32_t ring_res = 0, ring_slots = 0, ring_c = 0;
  bool ring_live = false;
  uint32_t *d_ring_of = nullptr, *d_ring_state = nullptr, *d_ring_src = nullptr, *d_ring_pay = nullptr;
  uint32_t* d_ring_next = nullptr;  // [0] slots handed out, [1] free-stack depth
  uint32_t* d_ring_free = nullptr;
  // ORSet-only full-state populations: the apply's work list for k_orset_merge
  uint4* d_orw = nullptr;
  uint2* d_orm = nullptr;
  uint32_t* d_orw_n = nullptr;
  // LWWMap engines (agx_set_lwwmap): the LWWRegister clock; d_lww_step0 = the supersteps with mail that ran
  // before the replay being launched (k_lwwmap_merge's logical time; written stream-ordered, run_single)
  uint32_t lww_clock = AGX_LWW_CLOCK_DEFAULT;
  uint32_t lww_delta_max = 0;  // LWWMap delta replication (agx_set_lwwmap_delta): max-delta-size, 0 = off (delta_max stays 0)
  uint64_t lww_base = 0;
  uint32_t* d_lww_step0 = nullptr;
  unsigned long long* d_ring_total = nullptr;
  uint32_t tstride = 4, region = 0;
  uint64_t acap = 0;  // arena capacity (fused: regions + overflow area)
  uint32_t apply_grid = kMaxApplyGrid;  // AGX_APPLY_GRID test knob: fewer blocks, each looping over buckets
  // blocks of the skew-list launch (grid-stride over the list; AGX_SKEW_GRID diagnostic knob): one
  // round of workgroups (2 per CU) -- an empty list at 10^8 actors cost 18 us with 4096 blocks
  uint32_t skew_grid = 512;
  bool stamps_skew = false;  // AGX_STAMPS_SKEW (diagnostic): phase stamps of the skew launch only
  std::vector<uint32_t> hd_key, hd_src, hd_pay;  // staged tells on the device, not yet consumed (fused)
  bool stg_pending = false;

  // host-staged tells (consumed by the next superstep)
  std::vector<uint32_t> hs_key, hs_src, hs_pay;
  uint32_t n_staged_dev = 0;  // staged tells uploaded for the next step
  uint64_t staged_total = 0, staged_dead = 0;
  uint64_t inflight_dev = 0;    // the device's in-flight count when inflight_known (agx_stage_tells' check)
  bool inflight_known = false;  // inflight_dev is current (cleared by every agx_run)
  bool last_run_ok = false;     // the last agx_run returned AGX_OK (agx_pump_idle's in-flight reschedule)
  bool tev1_recorded = false;   // agx_run_timed: run_single recorded the end event

  ncclComm_t comm = nullptr;
  bool started = false;
  // superstep graphs (single rank)
  static constexpr uint32_t kGraphSteps = 16;  // largest replay (kGraphSizes = 1, 2, 4, 8, 16); a replay boundary costs
                                              // ~18 us (graph launch + k_replay_out); with D2H copies per replay,
                                              // 16-superstep replays had measured slower (67 vs 24.7 us/superstep)
  bool graphs_enabled = true;
  // gx[strict][parity][size]: replays of kGraphSizes[size] supersteps; fused graphs exist per
  // starting parity (the parity is a kernel argument), multi-pass ones use gx[0][0][*].  A budget
  // of K supersteps replays its binary decomposition (20 = 8 + 8 + 4), never a run of singles.
  static constexpr uint32_t kNSizes = 5;
  hipGraphExec_t gx[2][2][kNSizes] = {};
  bool gx_persist[2][2][kNSizes] = {};  // that replay is one persistent launch (capture_steps)
  uint64_t persist_launches = 0, persist_supersteps = 0;  // replays launched as persistent launches (agx_persist_info)
  // multi-rank device-resident replays (run_multi_rccl): kMrReplay supersteps -- phase 1, the count
  // all-gather, k_mr_pack, the slab sends / receives, unpack, bucket passes, apply -- captured once as
  // one graph (RCCL collectives are captured with the kernels); mr_graph_ok cleared when a capture
  // fails (the replays then stay eager).  Opt-in: AGX_MR_GRAPH=1 (see run_multi_rccl).
  hipGraphExec_t mr_gx = nullptr;
  bool mr_graph_ok = true;
  // fused "strict" replays: graphs without the (usually empty) skew-list launches.  A superstep that
  // defers a skewed bucket marks d_abort; the rest of the replay is void and run_single runs the
  // deferred skew launch, then continues with the full graphs (strict_ok cleared for this engine).
  uint32_t* d_abort = nullptr;  // [2] (BucketArgs::abort)
  // persistent fused supersteps (k_dense_fused<.., true>): a captured replay of K dense-alone strict
  // supersteps is ONE launch with a grid barrier between supersteps (opt-in, AGX_PERSIST=1; default: K launches)
  int persist = -1;              // -1 not decided yet, 0 off (knob, too many buckets, a barrier timeout), 1 on
  uint32_t persist_steps = 0;    // capture_steps -> launch_apply: supersteps of the persistent launch
  uint32_t persist_vid = ~0u;    // the apply variant `persist` was decided for
  bool captured_persist = false; // the last capture_steps was one persistent launch
  uint32_t* d_pbar = nullptr;    // [4] grid barrier: arrivals, generation, timed out
  uint32_t* h_abort = nullptr;  // pinned [kLag][2]: the marks after each replay (eager path)
  // fused graphs end with k_replay_out, which writes the replay's inbox-size rows and abort marks
  // straight into the pinned host ring (device-mapped) at ring slot (replay counter % kLag): no
  // D2H copy between replays (those cost ~26 us per replay boundary, rocprofv3 kernel trace)
  uint32_t* d_ring = nullptr;   // device pointer of h_cntb
  uint32_t* d_rctr = nullptr;   // device replay counter (k_replay_out)
  uint64_t replay_ctr = 0;      // host mirror: fused graph replays launched
  bool strict_ok = true;        // AGX_NO_STRICT=1 disables
  bool strict_env = true;       // (the AGX_NO_STRICT knob; strict_ok is re-armed after clean replays)
  uint32_t clean_steps = 0;     // fused supersteps since the last skewed bucket (full graphs)
  uint32_t max_replay_si = 4;   // largest replay used: kGraphSizes[max_replay_si] (AGX_MAX_REPLAY knob)
  hipEvent_t lag_ev[4] = {};    // run_single's replay events (created once)
  bool strict_cap = false;      // the superstep being launched / captured is strict
  bool skew_only = false;       // recovery: the deferred skew launch alone
  unsigned long long* d_dbg = nullptr;  // AGX_STAMPS diagnostic build only

  // profiling
  bool prof = false;
  struct Rec { int cls; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  double prof_ms[K_NCLASS] = {0};
  uint64_t prof_n[K_NCLASS] = {0};
  // profiled dense launches (K_DENSE) that took every bucket, read from the device's dense_left words
  // after the launch: the wave / block launches after them returned at entry (agx_profile_read items)
  uint64_t prof_items[K_NCLASS] = {0};
};

namespace {

// The actor features, host side: one row per feature.  The top-level ones exclude one another, a multi-rank engine,
// CRDT kinds and a ring pool, and are set before the first run; such an engine launches the feature's instantiation
// of a catch-all k_bucket_apply (agx_launch_apply_feature) and no wave / ring / dense / persistent launch.  What is
// the same for every feature reads this table: the setters' common refusals (refuse_feature), enable_crdt's,
// apply_variant, launch_apply and make_params.
enum Feature : uint32_t { F_PRIO, F_STASH, F_TIMERS, F_WATCH, F_SUPER, F_CHILD, F_SHARD, F_IDLE, F_RECEP, F_ASK, F_LIST, F_TOPIC, F_HASH, F_BACKOFF, F_N, F_NONE = F_N };

struct FeatureRow {
  bool (*on)(const agx_engine*);
  const void* (*storage)(const agx_engine*);  // what stands in DevParams' shared slot (rx's)
  const char* needs;       // its refusals' subject and verb
  const char* named;       // as the other party of another feature's refusal
  const char* crdt_named;  // as the other party of enable_crdt's refusal
  const char* crdt_why;    // the reason tail of both CRDT refusals
  const char* emit_why;    // the reason tail of the max_emit refusal (null: any max_emit)
  const char* ring_why;    // the ring-pool refusal, between "rings of %u slots, " and " before the first run"
  const char* set_what;    // "set <set_what> before the first agx_run"
  uint32_t km;             // the launch: its KM flag bits ...
  bool prio;               // ... or kPrio
  Feature on_top_of;       // the feature it is set on top of (F_NONE: a top-level feature)
};

#define AGX_ONCE "the drain for more evaluates a case more than once, and "
const FeatureRow kFeatures[F_N] = {
    {[](const agx_engine* e) { return e->prio_mask != 0; }, [](const agx_engine* e) -> const void* { return e->d_ptab; },
     "priority mailboxes need", "priority tables (agx_set_mailbox_priority)", "a priority mailbox (agx_set_mailbox_priority)",
     ": a state gossip's snapshot handle carries no message tag", nullptr,
     "drained in arrival order: set priority tables", "mailbox priorities", 0, true, F_NONE},
    {[](const agx_engine* e) { return e->stash_on; }, [](const agx_engine* e) -> const void* { return e->d_stash; },
     "deque-based mailboxes need", "a deque-based mailbox class (agx_set_stash)", "a deque-based mailbox (agx_set_stash)",
     ": a state gossip's snapshot row does not outlive its superstep in a stash",
     "a stash drain stages at most one tell per message", "which know no stash: set stash capacities", "stash capacities",
     kStashKM, false, F_NONE},
    {[](const agx_engine* e) { return e->tm_keys != 0; }, [](const agx_engine* e) -> const void* { return e->d_timers; },
     "timers need", "timers (agx_set_timers)", "timers (agx_set_timers)", "", AGX_ONCE "a timer action must take effect once",
     "which know no timers: set timers", "timers", kTimersKM, false, F_NONE},
    {[](const agx_engine* e) { return e->wd_slots != 0; }, [](const agx_engine* e) -> const void* { return e->d_watch; },
     "death watch needs", "death watch (agx_set_death_watch)", "death watch (agx_set_death_watch)", "",
     AGX_ONCE "a watch action must take effect once", "which know no death watch: set death watch", "death watch", kWatchKM,
     false, F_NONE},
    {[](const agx_engine* e) { return e->sv_on; }, [](const agx_engine* e) -> const void* { return e->d_super; },
     "supervision needs", "supervision (agx_set_supervision)", "supervision (agx_set_supervision)", "",
     AGX_ONCE "a failure must take effect once", "which know no supervision: set supervision", "supervision", kSuperKM, false,
     F_NONE},
    // children (agx_set_children) come on top of death watch, whose storage holds theirs and whose refusals are
    // theirs: the row only selects the launch
    {[](const agx_engine* e) { return e->d_child != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kWatchKM | kChildKM, false, F_WATCH},
    // sharded entities (agx_set_sharding) come on top of receive timeouts, which come on top of the timers: the row
    // stands before theirs, so launched_feature (the first row that is on) selects the sharding instantiation
    {[](const agx_engine* e) { return e->d_shard != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kTimersKM | kIdleKM | kShardKM, false, F_TIMERS},
    // receive timeouts (agx_set_receive_timeout) come on top of the timers in the same way
    {[](const agx_engine* e) { return e->rt_on; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     kTimersKM | kIdleKM, false, F_TIMERS},
    {[](const agx_engine* e) { return e->d_recep != nullptr; }, [](const agx_engine* e) -> const void* { return e->d_recep; },
     "the receptionist needs", "the receptionist (agx_set_receptionist)", "the receptionist (agx_set_receptionist)", "",
     AGX_ONCE "a route must take effect once", "which know no receptionist: set the receptionist", "the receptionist",
     kRecepKM, false, F_NONE},
    // the ask pattern (agx_set_ask) comes on top of the timers as receive timeouts do; the two exclude one another
    {[](const agx_engine* e) { return e->ask_on; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     kTimersKM | kAskKM, false, F_TIMERS},
    // Subscribe / Listing (agx_set_listings) comes on top of topics, which come on top of the receptionist: its row
    // stands before theirs, so launched_feature (the first row that is on) selects the listings instantiation
    {[](const agx_engine* e) { return e->d_list != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kRecepKM | kTopicKM | kListKM, false, F_RECEP},
    // pub-sub topics (agx_set_topics) come on top of the receptionist in the same way
    {[](const agx_engine* e) { return e->d_topic != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kRecepKM | kTopicKM, false, F_RECEP},
    // consistent-hashing and random routing (agx_set_router_logics) come on top of the receptionist too; they and
    // topics exclude one another
    {[](const agx_engine* e) { return e->d_hash != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kRecepKM | kHashKM, false, F_RECEP},
    // restartWithBackoff (agx_set_backoff) comes on top of supervision, the only row there: launched_feature selects
    // the backoff instantiation for such an engine, and an engine that never calls agx_set_backoff launches what it did
    {[](const agx_engine* e) { return e->d_backoff != nullptr; }, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
     nullptr, kSuperKM | kBackoffKM, false, F_SUPER},
};
#undef AGX_ONCE

// the engine's top-level feature (at most one is on: refuse_feature), F_NONE without one
Feature active_feature(const agx_engine* e) {
  for (uint32_t f = 0; f < F_N; ++f)
    if (kFeatures[f].on_top_of == F_NONE && kFeatures[f].on(e)) return (Feature)f;
  return F_NONE;
}

// the feature whose instantiation the engine launches: `a`, or the one set on top of it
Feature launched_feature(const agx_engine* e, Feature a) {
  for (uint32_t f = 0; f < F_N; ++f)
    if (a != F_NONE && kFeatures[f].on_top_of == a && kFeatures[f].on(e)) return (Feature)f;
  return a;
}

// What every setter of a top-level feature refuses, after its own argument checks: more than one rank, CRDT kinds,
// another feature, max_emit, a ring pool (all AGX_EINVAL), and only then a started engine (AGX_ESTATE).
agx_status refuse_feature(const agx_engine* e, Feature f) {
  const FeatureRow& F = kFeatures[f];
  if (e->R > 1) return set_err(AGX_EINVAL, "%s a single-rank engine (n_ranks is %u; the limit is 1)", F.needs, e->R);
  if (e->pw) return set_err(AGX_EINVAL, "%s an engine without CRDT kinds (one is registered)%s", F.needs, F.crdt_why);
  const Feature a = active_feature(e);
  if (a != F_NONE && a != f) return set_err(AGX_EINVAL, "%s an engine without %s", F.needs, kFeatures[a].named);
  if (F.emit_why && e->kmax != 1)
    return set_err(AGX_EINVAL, "%s max_emit = 1 (it is %u): %s", F.needs, e->kmax, F.emit_why);
  if (e->ring_live || e->rg_on)
    return set_err(AGX_EINVAL, "this engine keeps queued messages in bounded-mailbox rings of %u slots, %s before the "
                   "first run", e->ring_live ? e->ring_c : e->rg_c, F.ring_why);
  if (e->started) return set_err(AGX_ESTATE, "set %s before the first agx_run", F.set_what);
  return AGX_OK;
}

agx_status ensure_dev(agx_engine* e) {
  HIP_TRY(hipSetDevice((int)e->cfg.device));
  return AGX_OK;
}

template <typename T>
agx_status dalloc(T** p, uint64_t n) {
  if (n == 0) n = 1;
  HIP_TRY(hipMalloc((void**)p, n * sizeof(T)));
  return AGX_OK;
}

// CRDT row storage (the snapshot heap and the multi-rank row buffers).  AGX_HEAP_POISON=<0..255>
// (test knob): every fresh allocation is filled with that byte, so a reader of a row word that no
// writer wrote sees the same value on every run instead of whatever the allocator handed out.
// Unset: hipMalloc alone, no further device call.
agx_status dalloc_rows(uint32_t** p, uint64_t n) {
  AGX_TRY(dalloc(p, n));
  if (const char* s = getenv("AGX_HEAP_POISON"))
    HIP_TRY(hipMemset(*p, std::min(255, std::max(0, atoi(s))), std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
  return AGX_OK;
}

agx_status alloc_msgs(DevMsgs& m, uint64_t n) {
  AGX_TRY(dalloc(&m.key, n));
  AGX_TRY(dalloc(&m.src, n));
  AGX_TRY(dalloc(&m.pay, n));
  return AGX_OK;
}

void free_msgs(DevMsgs& m) {
  hipFree(m.key);
  hipFree(m.src);
  hipFree(m.pay);
  m = DevMsgs{};
}

// --------------------------------------------------------------- profiling
void prof_begin(agx_engine* e, int cls, hipEvent_t* out_b) {
  *out_b = nullptr;
  if (!e->prof) return;
  if (e->ev_used + 2 > e->ev_pool.size()) {
    if (e->ev_pool.size() >= 200000) return;
    for (int i = 0; i < 1024; ++i) {
      hipEvent_t ev;
      if (hipEventCreate(&ev) != hipSuccess) return;
      e->ev_pool.push_back(ev);
    }
  }
  hipEvent_t a = e->ev_pool[e->ev_used++], b = e->ev_pool[e->ev_used++];
  hipEventRecord(a, e->stream);
  e->recs.push_back({cls, a, b});
  *out_b = b;
}
void prof_end(agx_engine* e, hipEvent_t b) {
  if (b) hipEventRecord(b, e->stream);
}
void prof_collect(agx_engine* e) {
  if (e->recs.empty()) return;
  hipStreamSynchronize(e->stream);
  for (auto& r : e->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      e->prof_ms[r.cls] += ms;
      e->prof_n[r.cls] += 1;
    }
  }
  e->recs.clear();
  e->ev_used = 0;
}

struct Scope {
  agx_engine* e;
  hipEvent_t b;
  Scope(agx_engine* e_, int cls) : e(e_) { prof_begin(e, cls, &b); }
  ~Scope() { prof_end(e, b); }
};

void drop_graphs(agx_engine* e);

DevParams make_params(agx_engine* e) {
  DevParams P{};
  P.n_global = (uint32_t)e->n_global;
  P.n_local = (uint32_t)e->n_local;
  P.W = e->W;
  P.T = e->T;
  P.C = e->C;
  P.Tr = e->Traw;
  P.nmc = e->mclasses ? 1u : 0u;
  for (uint32_t c = 0; c < AGX_MAX_MAILBOX_CLASSES; ++c) P.mcap[c] = e->mcap[c];
  P.pmask = e->prio_mask;
  P.host_lo = e->host_lo;
  P.host_n = e->host_n;
  P.outbox = e->d_outbox;
  P.outbox_n = e->d_outbox_n;
  P.outbox_cap = (uint32_t)e->outbox_cap;
  P.R = e->R;
  P.rank = e->rank;
  P.kmax = e->kmax;
  P.ring_stride = (uint32_t)(e->ring_stride % e->n_global);
  P.fan_k = e->fan_k;
  P.fan_seed = e->fan_seed;
  P.zipf_n = e->zipf_n;
  P.zipf_cdf = e->d_zcdf;
  P.zipf_ent = e->d_zent;
  P.zipf_perm = e->d_zperm;
  P.row_ptr = e->d_row;
  P.col = e->d_col;
  P.route = e->d_route;
  P.gid = e->d_gid;
  P.kind = e->d_kind;
  P.alive = e->d_alive;
  P.state = e->d_state;
  P.pitch = e->pitch;
  P.sa = e->pitch ? e->pitch : 1u;
  P.sw = e->pitch ? 1u : (uint32_t)e->n_local;
  P.stopq = e->d_stopq;
  P.nstop = e->d_nstop;
  P.heap = e->d_heap;
  P.rx = e->d_rx;
  // (a feature's storage shares rx's slot -- ptab, stash, timers, watch, super: no CRDT kinds on such an engine)
  if (const Feature f = active_feature(e); f != F_NONE) P.rx = static_cast<const uint32_t*>(kFeatures[f].storage(e));
  P.heap_top = e->d_heap_top;
  P.step = e->d_step;
  P.heap_rows = (uint32_t)e->heap_rows;
  P.pw = e->pw;
  P.gossip_f = e->gossip_f;
  P.gossip_seed = e->gossip_seed;
  P.delta_max = e->delta_max ? e->delta_max : e->lww_delta_max;  // (never both: agx_set_lwwmap_delta)
  P.bcase = e->d_bcase;
  P.bact = e->d_bact;
  P.bfirst = e->d_bfirst;
  P.n_beh = e->n_beh;
  P.err = reinterpret_cast<unsigned long long*>(e->d_stats + ST_ERROR);
  return P;
}

uint32_t grid_for(uint64_t tiles, uint32_t cap) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, cap)); }

// ------------------------------------------------------------ kernel steps
bool bypass_mode(const agx_engine* e) { return !e->fused && e->R == 1; }
// single-rank multi-pass: the tell arena the superstep of parity `par` writes
const DevMsgs& em_arena(const agx_engine* e, uint32_t par) { return par ? e->em2 : e->em; }

Chunks make_chunks(agx_engine* e) {
  Chunks c{};
  c.bl = e->bl.c();
  c.em = bypass_mode(e) ? em_arena(e, e->par ^ 1u).c() : e->em.c();  // (the previous apply's tells)
  c.st = e->stg.c();
  c.off = e->d_chunk_off;
  c.cnt = e->d_chunk_cnt;
  c.nb = e->nb;
  return c;
}

// one dense LSD pass (reduce-then-scan) over `bits` bits at `shift`
agx_status launch_dense_pass(agx_engine* e, const DevMsgs& in, const DevMsgs& out, const uint32_t* d_n, uint32_t shift,
                             uint32_t bits) {
  SortArgs sa{};
  sa.in = in.c();
  sa.out = out.m();
  sa.d_n = d_n;
  sa.hist = e->d_hist_d;
  sa.tot = e->d_tot;
  sa.bstart = e->d_bstart;
  sa.stride = e->dstride;
  sa.maxsub = e->dsub;
  sa.shift = shift;
  sa.bits = bits;
  // (multi-rank: the device-resident replays' stop word -- [0] != 0 makes the pass return, like identity)
  sa.ident = e->ident_on ? e->d_ident : e->R > 1 ? e->d_halt : nullptr;
  const uint32_t g = grid_for(e->max_supers, 4096);
  {
    Scope s(e, K_UPSWEEP);
    hipLaunchKernelGGL(k_sort_upsweep, dim3(g), dim3(kThreads), 0, e->stream, sa);
  }
  {
    Scope s(e, K_ROWSCAN);
    hipLaunchKernelGGL(k_sort_rowscan, dim3(1u << bits), dim3(kThreads), 0, e->stream, sa);
  }
  {
    Scope s(e, K_DOWNSWEEP);
    hipLaunchKernelGGL(k_sort_downsweep, dim3(g), dim3(kThreads), 0, e->stream, sa);
  }
  HIP_TRY(hipGetLastError());
  return AGX_OK;
}

// Group the mail by bucket.  first_from_chunks: pass 0 reads the chunk list written
// by the previous k_bucket_apply (single rank); otherwise every pass reads the dense A.
// Returns the buffer holding the result.
agx_status launch_bucket_sort(agx_engine* e, bool first_from_chunks, DevMsgs** result) {
  DevMsgs* src = &e->A;
  DevMsgs* dst = &e->B;
  uint32_t p0 = 0;
  if (first_from_chunks) {
    ChunkSortArgs ca{};
    ca.ch = make_chunks(e);
    ca.out = e->A.m();
    ca.hist = e->d_hist_c;
    ca.tot = e->d_tot;
    ca.d_n = e->d_n;
    ca.bstart = e->d_bstart;
    ca.stats = e->d_stats;
    ca.alive = e->d_alive;
    ca.stopq = e->d_stopq;
    ca.nstop = e->d_nstop;
    ca.step = e->d_step;  // superstep counter: CRDT heap parity and the backlog arena parity
    ca.blpre = e->d_blpre;
    ca.bl_stot = e->d_blpre + e->nb;
    ca.bl_sbase = e->d_blpre + e->nb + kMaxBlSlices;
    ca.d_ninbox = e->d_ninbox;
    ca.ring_total = e->ring_live || e->rg_on ? e->d_ring_total : nullptr;
    ca.bypass = 1;
    ca.heap_top = e->d_heap_top;
    ca.skew_n = e->d_skew_n;
    ca.cap = e->cap;
    ca.stride = e->cstride;
    ca.nunits = e->nunits;
    ca.ng = e->ng;
    ca.G = e->G;
    ca.shift = e->plan.shift[0];
    ca.bits = e->plan.bits[0];
    const uint32_t nsl = (e->nb + kBlSlice - 1) / kBlSlice;
    if (e->ident_on) {
      ca.emmeta = e->d_emmeta;
      ca.slsum = e->d_slsum;
      ca.ident = e->d_ident;
    }
    {
      Scope s(e, K_CROWSCAN);
      if (e->ident_on && e->plan.npass > 1) {
        // the decision first (slice summaries, k_ident_combine), then the rowscan proper, whose digit
        // rows are skipped under identity (k_bucket_bounds finds the bucket starts in place)
        ca.part = 1;
        hipLaunchKernelGGL(k_chunk_rowscan, dim3(nsl + 1), dim3(kThreads), 0, e->stream, ca);
        hipLaunchKernelGGL(k_ident_combine, dim3(1), dim3(kWave), 0, e->stream, e->d_slsum, nsl, e->d_ident,
                           reinterpret_cast<unsigned long long*>(e->d_stats + ST_IDENT));
        ca.part = 2;
        hipLaunchKernelGGL(k_chunk_rowscan, dim3((1u << ca.bits) + nsl), dim3(kThreads), 0, e->stream, ca);
      } else {
        hipLaunchKernelGGL(k_chunk_rowscan, dim3((1u << ca.bits) + nsl + (e->ident_on ? nsl + 1 : 0)), dim3(kThreads), 0,
                           e->stream, ca);
        if (e->ident_on)  // this superstep's grouping: identity (no pass) or the radix passes
          hipLaunchKernelGGL(k_ident_combine, dim3(1), dim3(kWave), 0, e->stream, e->d_slsum, nsl, e->d_ident,
                             reinterpret_cast<unsigned long long*>(e->d_stats + ST_IDENT));
      }
    }
    {
      Scope s(e, K_CDOWN);
      hipLaunchKernelGGL(k_chunk_downsweep, dim3(grid_for(e->nunits, 4096)), dim3(kThreads), 0, e->stream, ca);
    }
    HIP_TRY(hipGetLastError());
    p0 = 1;
  }
  for (uint32_t p = p0; p < e->plan.npass; ++p) {
    AGX_TRY(launch_dense_pass(e, *src, *dst, e->d_n, e->plan.shift[p], e->plan.bits[p]));
    std::swap(src, dst);
  }
  if (e->plan.npass > 1) {  // digits of the last pass are not buckets: find the bucket starts
    Scope s(e, K_BOUNDS);
    const bool idn = e->ident_on && first_from_chunks;
    hipLaunchKernelGGL(k_bucket_bounds, dim3(grid_for((e->nb + kThreads) / kThreads, 4096)), dim3(kThreads), 0,
                       e->stream, src->key, e->d_n, e->nb, e->bb, e->d_bstart, idn ? e->d_ident : nullptr,
                       idn ? em_arena(e, e->par ^ 1u).key : nullptr, e->R > 1 ? e->d_halt : nullptr);
    HIP_TRY(hipGetLastError());
  }
  *result = src;
  return AGX_OK;
}

// multi-pass, plain behaviours: partition the skewed buckets over workgroups before the skew
// launch (k_skew_plan / count / scan / scatter, agx_kernels.h); grids are fixed (graph capture),
// the kernels stride over the device-side part and bucket counts
void skew_prepass(agx_engine* e, const BucketArgs& ba, const SkewArgs& ska) {
  const uint32_t gp = std::min<uint32_t>(e->sk_rows, 1024), gb = grid_for(e->nb, kMaxApplyGrid);
  hipLaunchKernelGGL(k_skew_plan, dim3(1), dim3(kScanThreads), 0, e->stream, ba, ska);
  hipLaunchKernelGGL(k_skew_count, dim3(gp), dim3(kBThreads), 0, e->stream, ba, ska);
  hipLaunchKernelGGL(k_skew_scan, dim3(gb), dim3(kBThreads), 0, e->stream, ba, ska);
  hipLaunchKernelGGL(k_skew_scatter, dim3(gp), dim3(kBThreads), 0, e->stream, ba, ska);
}

// the k_bucket_apply variant for the registered behaviour kinds (agx_variants.h)
uint32_t apply_variant(const agx_engine* e) {
  const uint32_t km = e->kinds_mask & ~kb(AGX_KIND_NONE);
  // a feature: the compiled catch-all carries its code (its KM flags); both plain catch-alls carry the order step (kPrio)
  if (const Feature f = active_feature(e); f != F_NONE)
    return kFeatures[f].prio && !(km & kb(AGX_KIND_COMPILED)) ? V_ALL : V_ALL_COMPILED;
  if (e->pw && e->delta_max) {  // delta-CRDT replication: the variants that carry the delta code
    if (km == kb(AGX_KIND_GCOUNTER)) return V_GC_DELTA;
    if (km == kb(AGX_KIND_PNCOUNTER)) return V_PN_DELTA;
    if (km == kb(AGX_KIND_ORSET)) return V_OR_DELTA;
    return V_ALL_DELTA;
  }
  if (e->pw) {  // CRDT kinds registered: single-kind populations get specialised merges
    if (km == kb(AGX_KIND_GCOUNTER)) return V_GC;
    if (km == kb(AGX_KIND_PNCOUNTER)) return V_PN;
    if (km == kb(AGX_KIND_ORSET)) return V_OR;
    if (km == kb(AGX_KIND_LWWMAP))  // (an LWWMap engine holds nothing else: agx_register_range)
      return e->lww_delta_max ? V_LWWMAP_DELTA : V_LWWMAP;
    if (km == kb(AGX_KIND_PNCOUNTERMAP)) return V_PNCMAP;  // (nor does a PNCounterMap engine)
    if (km == kb(AGX_KIND_ORMULTIMAP)) return V_ORMM;      // (nor an ORMultiMap engine)
    if ((km & ~kCrdtKM) == 0) return V_CRDT;  // CRDT kinds only: no plain-behaviour code
    return V_ALL_WIDE;
  }
  if (km == kb(AGX_KIND_RING)) return V_RING;  // behaviour-specialised variants (see apply_msg)
  if (km == kb(AGX_KIND_FORWARD_RR)) return V_FWD;
  if (km == kb(AGX_KIND_FANOUT)) return V_FANOUT;
  if (km == kb(AGX_KIND_COUNTER)) return V_COUNTER;
  if (km == kb(AGX_KIND_COMPILED)) return V_COMPILED;  // compiled behaviours only (agx_set_behaviors)
  if (km & kb(AGX_KIND_COMPILED)) return V_ALL_COMPILED;
  return V_ALL;
}

// the lean dense-bucket launch before the block launch (k_dense_apply / k_dense_fused): plain
// behaviours, one tell per message, no bounded-mailbox rings; by default for ring populations
bool dense_on(const agx_engine* e, uint32_t vid) {
  const bool mode_ok = e->fused ? e->dense_fused : e->R == 1 || e->dense_owner;
  // (k_dense_fused reads a fused bucket's table row one sender bucket per thread: nb <= 512, which
  // the fused superstep's <= 2^20 actors guarantee)
  if (e->fused && e->nb > (uint32_t)kDenseThreads) return false;
  return mode_ok && !kVariants[vid].wide && e->kmax == 1 && !e->ring_live && active_feature(e) == F_NONE &&
         (e->dense_launch == 1 || (e->dense_launch < 0 && vid == V_RING));
}

// ---- the receptionist (agx_set_receptionist): the rebuild of the sorted listings between two
// supersteps.  apply -> k_recep_scan -> k_recep_fill -> the next apply are kernel boundaries: no polling between
// workgroups, no grid barrier; the listings are rebuilt in place, stream order keeps readers and the writer apart.
constexpr int kRcThreads = 256;
// One block per key; returns at entry when the key is neither dirty nor marked as rebuilt (one word read).  A dirty
// key: the exclusive scan of cnt[key][0..nb) into the per-bucket offsets, the size, the version, the capacity
// error; its dirty bit moves to dirty_now.
static __global__ void __launch_bounds__(kRcThreads) k_recep_scan(uint32_t* rc, unsigned long long* err) {
  const uint32_t k = blockIdx.x, f = rc[kRcFlags];
  const bool dirty = (f >> k) & 1u, now = (f >> (8u + k)) & 1u;
  if (!dirty && !now) return;
  if (!dirty) {  // rebuilt after the tick before: the mark goes
    if (threadIdx.x == 0) atomicAnd(rc + kRcFlags, ~(1u << (8u + k)));
    return;
  }
  const RecepDev RD = recep_dev(rc);
  __shared__ uint32_t scratch[kRcThreads / kWave + 1];
  uint32_t run = 0;
  for (uint32_t b0 = 0; b0 < RD.nb; b0 += kRcThreads) {  // (block-uniform trip count)
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t c = b < RD.nb ? *RD.cnt(k, b) : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_sum<kRcThreads>(c, scratch, &tot);
    if (b < RD.nb) *RD.off(k, b) = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) {
    if (run > RD.cap) atomicOr(err, (unsigned long long)kErrRecepCap);  // (k_recep_fill writes the first `capacity` ids)
    rc[kRcSize + k] = min(run, RD.cap);
    reinterpret_cast<unsigned long long*>(rc + kRcVersion)[k] += 1ull;
    atomicAdd(RD.ctr(kRcRebuilds), 1ull);
    atomicOr(rc + kRcFlags, 1u << (8u + k));
    atomicAnd(rc + kRcFlags, ~(1u << k));
  }
}
// One block per bucket; returns at entry when no key is being rebuilt (one word read).  Else the bucket's members
// of each such key go to the key's listing at the bucket's offset, in ascending id: ballot and lane rank within a
// wave, the waves' counts through LDS.
static __global__ void __launch_bounds__(kRcThreads) k_recep_fill(uint32_t* rc, uint32_t bb, uint32_t n_local) {
  uint32_t now = (rc[kRcFlags] >> 8) & 0xFFu;
  if (!now) return;
  const RecepDev RD = recep_dev(rc);
  now &= (1u << RD.nk) - 1u;
  constexpr uint32_t kW = kRcThreads / kWave;
  __shared__ uint32_t s_wc[AGX_MAX_SERVICE_KEYS][kW];
  const uint32_t tid = threadIdx.x, w = tid / kWave, b = blockIdx.x, a0 = b << bb;
  const uint32_t na = min(1u << bb, n_local - a0);
  const uint64_t lt = lanemask_lt();
  uint32_t run[AGX_MAX_SERVICE_KEYS] = {};
  for (uint32_t c0 = 0; c0 < na; c0 += kRcThreads) {  // (block-uniform trip count)
    const uint32_t la = c0 + tid;
    const uint32_t m = la < na ? RD.mask[a0 + la] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
      if (!((now >> k) & 1u)) continue;
      const uint64_t bal = __ballot((m >> k) & 1u);
      if (lane_id() == 0) s_wc[k][w] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
      if (!((now >> k) & 1u)) continue;
      const uint64_t bal = __ballot((m >> k) & 1u);
      uint32_t pre = 0, tot = 0;
#pragma unroll
      for (uint32_t i = 0; i < kW; ++i) {
        const uint32_t t = s_wc[k][i];
        pre += i < w ? t : 0u;
        tot += t;
      }
      if ((m >> k) & 1u) {
        const uint32_t pos = *RD.off(k, b) + run[k] + pre + (uint32_t)__popcll(bal & lt);
        if (pos < RD.cap) RD.list(k)[pos] = a0 + la;
      }
      run[k] += tot;
    }
    __syncthreads();  // (s_wc is rewritten by the next chunk)
  }
}
// agx_register_services on the device: one block per bucket the range touches sets or clears bit `key` of the
// range's live actors, recounts the bucket's members of the key and marks the key dirty if a bit changed
static __global__ void __launch_bounds__(kRcThreads) k_recep_start(uint32_t* rc, const uint8_t* alive, uint32_t bb, uint32_t n_local,
                                                                   uint32_t first, uint32_t count, uint32_t key, uint32_t on,
                                                                   uint32_t b_first) {
  const RecepDev RD = recep_dev(rc);
  const uint32_t tid = threadIdx.x, b = b_first + blockIdx.x, a0 = b << bb, bit = 1u << key;
  const uint32_t na = min(1u << bb, n_local - a0);
  __shared__ uint32_t s_n[3];  // members, bits set, bits cleared
  if (tid < 3) s_n[tid] = 0u;
  __syncthreads();
  uint32_t members = 0, nset = 0, nclr = 0;
  for (uint32_t la = tid; la < na; la += kRcThreads) {
    const uint32_t l = a0 + la;
    uint32_t m = RD.mask[l];
    if (l >= first && l - first < count && (alive[l] & 1u)) {
      const uint32_t m2 = on ? m | bit : m & ~bit;
      if (m2 != m) {
        RD.mask[l] = (uint8_t)m2;
        nset += on ? 1u : 0u;
        nclr += on ? 0u : 1u;
        m = m2;
      }
    }
    members += (m >> key) & 1u;
  }
  if (members) atomicAdd(&s_n[0], members);
  if (nset) atomicAdd(&s_n[1], nset);
  if (nclr) atomicAdd(&s_n[2], nclr);
  __syncthreads();
  if (tid == 0) {
    *RD.cnt(key, b) = s_n[0];
    if (s_n[1]) atomicAdd(RD.ctr(kRcRegistered), (unsigned long long)s_n[1]);
    if (s_n[2]) atomicAdd(RD.ctr(kRcDeregistered), (unsigned long long)s_n[2]);
    if (s_n[1] | s_n[2]) atomicOr(rc + kRcFlags, bit);
  }
}

// ---- consistent-hashing routing (agx_set_router_logics): the rings of the hashed keys being rebuilt
// (dirty_now after k_recep_scan, or `force`) are rewritten as the stable compaction of the static ring by the key's
// mask bit.  k_recep_fill -> k_hash_count -> k_hash_scan -> k_hash_fill -> the next apply are kernel boundaries.
// Each kernel returns at entry when no hashed key is being rebuilt (one flags word and the header read).
static_assert(kHrSeg % kRcThreads == 0, "a segment is whole chunks of one block");
__device__ __forceinline__ uint32_t hash_keys_now(const uint32_t* rc, const uint32_t* hb, uint32_t force) {
  return (((rc[kRcFlags] >> 8) & 0xFFu) | force) & hb[kHrMask];
}
// One block per segment of the static ring: the segment's members of each such key (a gather of one mask byte per point)
static __global__ void __launch_bounds__(kRcThreads) k_hash_count(uint32_t* rc, uint32_t force) {
  uint32_t* const hb = hash_base_of(rc);
  const uint32_t now = hash_keys_now(rc, hb, force);
  if (!now) return;
  const RecepDev RD = recep_dev(rc);
  const HashDev HD = hash_dev(hb);
  __shared__ uint32_t s_c[AGX_MAX_SERVICE_KEYS];
  const uint32_t tid = threadIdx.x, s = blockIdx.x, p0 = s * kHrSeg;
  if (tid < AGX_MAX_SERVICE_KEYS) s_c[tid] = 0u;
  __syncthreads();
  const uint32_t* const sid = HD.st_id();
  uint32_t cnt[AGX_MAX_SERVICE_KEYS] = {};
  for (uint32_t c0 = 0; c0 < kHrSeg; c0 += kRcThreads) {
    const uint32_t p = p0 + c0 + tid;
    const uint32_t m = p < HD.npts ? RD.mask[sid[p]] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) cnt[k] += (m >> k) & 1u;
  }
#pragma unroll
  for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
    if (!((now >> k) & 1u)) continue;  // (block-uniform)
    const uint32_t t = wave_incl_sum(cnt[k]);
    if (lane_id() == kWave - 1 && t) atomicAdd(&s_c[k], t);
  }
  __syncthreads();
  if (tid < AGX_MAX_SERVICE_KEYS && ((now >> tid) & 1u)) HD.segcnt(HD.slot(tid))[s] = s_c[tid];
}
// One block per key: the exclusive scan of the key's segment counts into the segment offsets, the ring's size
static __global__ void __launch_bounds__(kRcThreads) k_hash_scan(uint32_t* rc, uint32_t force) {
  uint32_t* const hb = hash_base_of(rc);
  const uint32_t k = blockIdx.x;
  if (!((hash_keys_now(rc, hb, force) >> k) & 1u)) return;
  const HashDev HD = hash_dev(hb);
  const uint32_t sl = HD.slot(k);
  __shared__ uint32_t scratch[kRcThreads / kWave + 1];
  uint32_t run = 0;
  for (uint32_t s0 = 0; s0 < HD.nseg; s0 += kRcThreads) {  // (block-uniform trip count)
    const uint32_t s = s0 + threadIdx.x;
    const uint32_t c = s < HD.nseg ? HD.segcnt(sl)[s] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_sum<kRcThreads>(c, scratch, &tot);
    if (s < HD.nseg) HD.segoff(sl)[s] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) {
    hb[kHrSize + k] = run;
    if (!((force >> k) & 1u)) atomicAdd(HD.ctr(kHrRebuilds), 1ull);  // (not the first build of the setter)
  }
}
// One block per segment: the segment's members of each such key go to the key's ring at the segment's offset, in the
// static ring's order: ballot and lane rank within a wave, the waves' counts through LDS (as k_recep_fill)
static __global__ void __launch_bounds__(kRcThreads) k_hash_fill(uint32_t* rc, uint32_t force) {
  uint32_t* const hb = hash_base_of(rc);
  const uint32_t now = hash_keys_now(rc, hb, force);
  if (!now) return;
  const RecepDev RD = recep_dev(rc);
  const HashDev HD = hash_dev(hb);
  constexpr uint32_t kW = kRcThreads / kWave;
  __shared__ uint32_t s_wc[AGX_MAX_SERVICE_KEYS][kW];
  const uint32_t tid = threadIdx.x, w = tid / kWave, s = blockIdx.x, p0 = s * kHrSeg;
  const uint64_t lt = lanemask_lt();
  const uint32_t* const sh = HD.st_hash();
  const uint32_t* const sid = HD.st_id();
  uint32_t run[AGX_MAX_SERVICE_KEYS] = {};
  for (uint32_t c0 = 0; c0 < kHrSeg; c0 += kRcThreads) {  // (block-uniform trip count)
    const uint32_t p = p0 + c0 + tid;
    const uint32_t id = p < HD.npts ? sid[p] : 0u;
    const uint32_t m = p < HD.npts ? RD.mask[id] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
      if (!((now >> k) & 1u)) continue;
      const uint64_t bal = __ballot((m >> k) & 1u);
      if (lane_id() == 0) s_wc[k][w] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
      if (!((now >> k) & 1u)) continue;
      const uint64_t bal = __ballot((m >> k) & 1u);
      uint32_t pre = 0, tot = 0;
#pragma unroll
      for (uint32_t i = 0; i < kW; ++i) {
        const uint32_t t = s_wc[k][i];
        pre += i < w ? t : 0u;
        tot += t;
      }
      if ((m >> k) & 1u) {
        const uint32_t sl = HD.slot(k);
        const uint32_t pos = HD.segoff(sl)[s] + run[k] + pre + (uint32_t)__popcll(bal & lt);
        if (pos < HD.npts) {
          HD.ring_hash(sl)[pos] = sh[p];
          HD.ring_id(sl)[pos] = id;
        }
      }
      run[k] += tot;
    }
    __syncthreads();  // (s_wc is rewritten by the next chunk)
  }
}

void launch_hash_rebuild(agx_engine* e, uint32_t force) {
  if (!e->hr_nseg) return;  // (random routing only: no ring)
  hipLaunchKernelGGL(k_hash_count, dim3(e->hr_nseg), dim3(kRcThreads), 0, e->stream, e->d_recep, force);
  hipLaunchKernelGGL(k_hash_scan, dim3(e->rc_keys), dim3(kRcThreads), 0, e->stream, e->d_recep, force);
  hipLaunchKernelGGL(k_hash_fill, dim3(e->hr_nseg), dim3(kRcThreads), 0, e->stream, e->d_recep, force);
}

void launch_recep_rebuild(agx_engine* e) {
  hipLaunchKernelGGL(k_recep_scan, dim3(e->rc_keys), dim3(kRcThreads), 0, e->stream, e->d_recep,
                     reinterpret_cast<unsigned long long*>(e->d_stats + ST_ERROR));
  hipLaunchKernelGGL(k_recep_fill, dim3(e->nb), dim3(kRcThreads), 0, e->stream, e->d_recep, e->bb, (uint32_t)e->n_local);
  if (e->d_hash) launch_hash_rebuild(e, 0u);  // (the rings of the hashed keys that k_recep_scan marked)
}

// ---- pub-sub topics (agx_set_topics): the plan between two supersteps.  apply -> k_topic_plan -> the
// next apply are kernel boundaries: no polling between workgroups, no grid barrier; the drains of the apply only
// append to the staging area, the blocks of the next apply only read the log, their due word and their masks.
constexpr int kTpThreads = 1024;
// due[b] = sum over keys of pubs[key] x cnt[key][b] for every bucket, which joins the bucket's backlog count (`blc`:
// the counts the next apply reads); what the pending log adds to fanned_out / no_subscribers replaces what it
// added before (`replan`: the old due counts leave the backlog counts first).  Every thread of the block calls.
__device__ __forceinline__ void topic_due(const TopicDev& TP, const RecepDev& RD, uint32_t* blc, bool replan, uint32_t* s_mem,
                                          unsigned long long* s_fan) {
  const uint32_t tid = threadIdx.x;
  if (tid < AGX_MAX_SERVICE_KEYS) s_mem[tid] = 0u;
  if (tid == 0) *s_fan = 0ull;
  __syncthreads();
  uint32_t pubs[AGX_MAX_SERVICE_KEYS], mem[AGX_MAX_SERVICE_KEYS] = {};
#pragma unroll
  for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) pubs[k] = k < RD.nk ? TP.base[kTpPubs + k] : 0u;
  unsigned long long fan = 0ull;
  for (uint32_t b = tid; b < TP.nb; b += kTpThreads) {
    unsigned long long d = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
      if (pubs[k]) {  // (block-uniform)
        const uint32_t c = *RD.cnt(k, b);
        mem[k] += c;
        d += (unsigned long long)pubs[k] * c;
      }
    const uint32_t dn = (uint32_t)(d < kTpDueMax ? d : kTpDueMax), old = replan ? *TP.due(b) : 0u;
    *TP.due(b) = dn;
    if (dn | old) {
      const uint32_t x = blc[b];
      blc[b] = x - min(old, x) + dn;
    }
    fan += dn;
  }
#pragma unroll
  for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
    if (mem[k]) atomicAdd(&s_mem[k], mem[k]);
  if (fan) atomicAdd(s_fan, fan);
  __syncthreads();
  if (tid == 0) {
    unsigned long long nosub = 0ull;
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
      if (pubs[k] && !s_mem[k]) nosub += pubs[k];
    const unsigned long long f = *s_fan;
    *TP.ctr(kTpFannedOut) += f - *TP.last(0);      // (one block, one writer; wraps back when the plan shrinks)
    *TP.ctr(kTpNoSubscribers) += nosub - *TP.last(1);
    *TP.last(0) = f;
    *TP.last(1) = nosub;
  }
}
// One block, after every apply.  Nothing staged and no pending log: returns after one 16-byte load.  A pending log
// whose tick has not come (no bucket had mail in this superstep) stays.  Else the log is consumed: with nothing
// staged it is emptied; else the staged publications are ranked by (publisher, window index) into the log (each
// thread counts the entries before its own: n^2 / 1024 compares per thread, n <= log_capacity), counted per key,
// and planned (topic_due).  More staged than log_capacity: the sticky error, the log keeps log_capacity of them.
// replan != 0 (after agx_register_services / agx_publish between two runs): the pending log planned again.
static __global__ void __launch_bounds__(kTpThreads) k_topic_plan(uint32_t* rc, uint32_t* blc, unsigned long long* err,
                                                                  uint32_t replan) {
  const RecepDev RD = recep_dev(rc);
  const TopicDev TP = topic_dev_of(rc);
  const uint32_t tid = threadIdx.x;
  __shared__ uint32_t s_mem[AGX_MAX_SERVICE_KEYS], s_pubs[AGX_MAX_SERVICE_KEYS];
  __shared__ unsigned long long s_fan;
  const uint4 h = *reinterpret_cast<const uint4*>(TP.base + kTpCursor);  // cursor, mail, n_log
  if (replan) {
    if (h.z) topic_due(TP, RD, blc, true, s_mem, &s_fan);  // (block-uniform)
    return;
  }
  const uint32_t ns = h.x;
  if (!ns && (!h.z || !h.y)) return;
  const uint32_t n = min(ns, TP.cap);
  if (tid < AGX_MAX_SERVICE_KEYS) s_pubs[tid] = 0u;
  __syncthreads();
  const uint4* const st = TP.stage();
  uint4* const lg = TP.log();
  for (uint32_t i = tid; i < n; i += kTpThreads) {
    const uint4 me = st[i];
    const unsigned long long mk = ((unsigned long long)me.x << 32) | me.y;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {  // (a publisher's window indices differ: the keys are distinct)
      const uint4 o = st[j];
      rank += (((unsigned long long)o.x << 32) | o.y) < mk ? 1u : 0u;
    }
    lg[rank] = make_uint4(me.z, me.x, me.w, 0u);
    atomicAdd(&s_pubs[me.z & 7u], 1u);
  }
  __syncthreads();
  if (tid < AGX_MAX_SERVICE_KEYS) TP.base[kTpPubs + tid] = s_pubs[tid];
  if (tid == 0) {
    if (ns > TP.cap) atomicOr(err, (unsigned long long)kErrTopicLog);
    TP.base[kTpCursor] = 0u;
    TP.base[kTpMail] = 0u;
    TP.base[kTpNLog] = n;
    *TP.last(0) = 0ull;  // (a fresh log: nothing of it is counted yet)
    *TP.last(1) = 0ull;
  }
  __threadfence();
  __syncthreads();
  topic_due(TP, RD, blc, false, s_mem, &s_fan);
}
// agx_publish on the device: the publication joins the pending log after what the device left there
static __global__ void k_topic_host_pub(uint32_t* rc, uint32_t key, uint32_t sender, uint32_t payload, unsigned long long* err) {
  const TopicDev TP = topic_dev_of(rc);
  const uint32_t n = TP.base[kTpNLog];
  atomicAdd(TP.ctr(kTpHostPublished), 1ull);
  if (n >= TP.cap) {
    atomicOr(err, (unsigned long long)kErrTopicLog);
    return;
  }
  TP.log()[n] = make_uint4(key, sender, payload, 0u);
  TP.base[kTpNLog] = n + 1u;
  TP.base[kTpPubs + key] += 1u;
  TP.base[kTpMail] = 0u;  // (the log's tick is the next superstep with mail)
}

void launch_topic_plan(agx_engine* e, uint32_t* blc, uint32_t replan) {
  hipLaunchKernelGGL(k_topic_plan, dim3(1), dim3(kTpThreads), 0, e->stream, e->d_recep, blc,
                     reinterpret_cast<unsigned long long*>(e->d_stats + ST_ERROR), replan);
}

// ---- Subscribe / Listing (agx_set_listings): the plan between two supersteps, after k_recep_scan /
// k_recep_fill / k_topic_plan.  Kernel boundaries again: the drains of the apply store their own actors' sub and
// pending bytes and their bucket's counts, the blocks of the next apply read their due word, the changed-keys word and
// their own bytes.
// One block.  replan == 0, after every apply: the keys rebuilt in this superstep (the dirty_now bits of the
// receptionist's flags word) are the changes the next tick's Listings announce; they replace the word of the tick
// before if this superstep was a tick (its Listings were served), else they join it.  No rebuilt key, no new pending
// bit, no changed key waiting and nothing of a served plan to take back: returns after the header's 16-byte load and
// the flags word -- two small loads, not one -- and the mail mark may then stay set.  A stale mark is harmless: it
// only decides whether a waiting changed-keys word is replaced or joined, the early return needs that word to be
// empty, and a superstep without mail has no recipient to tell (agx_run launches no superstep on a quiescent engine;
// the empty supersteps at the tail of a replayed batch drain nothing).  Else due[b] = the sum over changed keys
// of cnt_u[k][b] plus the sum over the others of cnt_p[k][b], which joins the bucket's backlog count (`blc`: the
// counts the next apply reads).  replan != 0 (after host calls between two runs): the keys whose version moved since
// k_listing_mark join the word -- each change becomes deliveries once, however many rebuilds the host's calls ran and
// whichever dirty_now bits they left --, the old due counts leave the backlog counts, and what the plan added to
// listings_sent / notified before is replaced.
static __global__ void __launch_bounds__(kTpThreads) k_listing_plan(uint32_t* rc, uint32_t* blc, uint32_t replan) {
  const ListDev LD = list_dev_of(rc);
  const uint32_t tid = threadIdx.x;
  const uint4 h = *reinterpret_cast<const uint4*>(LD.base + kLsMail);  // mail, changed, pend, planned
  const uint32_t nkm = (1u << LD.nk) - 1u;
  uint32_t chg = h.y;
  if (replan) {
    for (uint32_t k = 0; k < LD.nk; ++k)  // (every thread reads the same words: broadcast loads)
      if (reinterpret_cast<const unsigned long long*>(rc + kRcVersion)[k] != *LD.seen(k)) chg |= 1u << k;
  } else {
    const uint32_t now = (rc[kRcFlags] >> 8) & nkm;
    if (!now && !h.y && !h.z && !h.w) return;
    chg = (h.x ? 0u : chg) | now;
  }
  __shared__ uint32_t s_rcp[AGX_MAX_SERVICE_KEYS];
  __shared__ unsigned long long s_sent;
  if (tid < AGX_MAX_SERVICE_KEYS) s_rcp[tid] = 0u;
  if (tid == 0) s_sent = 0ull;
  __syncthreads();
  if (replan || chg || h.z) {  // (block-uniform)
    uint32_t rcp[AGX_MAX_SERVICE_KEYS] = {};
    unsigned long long sent = 0ull;
    for (uint32_t b = tid; b < LD.nb; b += kTpThreads) {
      uint32_t d = 0;
#pragma unroll
      for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
        if (k < LD.nk) {  // (block-uniform)
          const bool c = (chg >> k) & 1u;
          const uint32_t n = c ? *LD.cnt_u(k, b) : *LD.cnt_p(k, b);
          if (c) rcp[k] += n;
          d += n;
        }
      const uint32_t old = replan ? *LD.due(b) : 0u;
      if (d | old) {
        *LD.due(b) = d;
        const uint32_t x = blc[b];
        blc[b] = x - min(old, x) + d;
      }
      sent += d;
    }
#pragma unroll
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
      if (rcp[k]) atomicAdd(&s_rcp[k], rcp[k]);
    if (sent) atomicAdd(&s_sent, sent);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long ntf = 0ull;
    for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) ntf += s_rcp[k] ? 1ull : 0ull;
    const unsigned long long l0 = replan ? *LD.last(0) : 0ull, l1 = replan ? *LD.last(1) : 0ull;
    *LD.ctr(kLsSent) += s_sent - l0;  // (one block, one writer; wraps back when the plan shrinks)
    *LD.ctr(kLsNotified) += ntf - l1;
    *LD.last(0) = s_sent;
    *LD.last(1) = ntf;
    LD.base[kLsChanged] = chg;
    LD.base[kLsPlanned] = (s_sent | ntf) != 0ull ? 1u : 0u;
    if (!replan) {
      LD.base[kLsMail] = 0u;
      LD.base[kLsPend] = 0u;
    } else {
      for (uint32_t k = 0; k < LD.nk; ++k) *LD.seen(k) = reinterpret_cast<const unsigned long long*>(rc + kRcVersion)[k];
    }
  }
}
// before the host's calls between two runs are applied: the versions as they stand (k_listing_plan's re-plan compares)
static __global__ void k_listing_mark(uint32_t* rc) {
  const ListDev LD = list_dev_of(rc);
  if (threadIdx.x < LD.nk) *LD.seen(threadIdx.x) = reinterpret_cast<const unsigned long long*>(rc + kRcVersion)[threadIdx.x];
}
// agx_subscribe_listings on the device: one block per bucket the range touches sets bit `key` of sub and pending
// (on) or clears it in sub (off) for the range's live actors, and recounts the bucket's two counts of the key
static __global__ void __launch_bounds__(kRcThreads) k_listing_start(uint32_t* rc, const uint8_t* alive, uint32_t bb, uint32_t n_local,
                                                                     uint32_t first, uint32_t count, uint32_t key, uint32_t on,
                                                                     uint32_t b_first) {
  const ListDev LD = list_dev_of(rc);
  const uint32_t tid = threadIdx.x, b = b_first + blockIdx.x, a0 = b << bb, bit = 1u << key;
  const uint32_t na = min(1u << bb, n_local - a0);
  __shared__ uint32_t s_n[3];  // sub | pending, pending, members changed by on
  if (tid < 3) s_n[tid] = 0u;
  __syncthreads();
  uint32_t nu = 0, np = 0, nc = 0;
  for (uint32_t la = tid; la < na; la += kRcThreads) {
    const uint32_t l = a0 + la;
    uint32_t sb = LD.sub[l], pd = LD.pend[l];
    if (l >= first && l - first < count && (alive[l] & 1u)) {
      const uint32_t sb2 = on ? sb | bit : sb & ~bit, pd2 = on ? pd | bit : pd;
      if (sb2 != sb) LD.sub[l] = (uint8_t)sb2;
      if (pd2 != pd) LD.pend[l] = (uint8_t)pd2;
      nc += (on && (sb2 != sb || pd2 != pd)) ? 1u : 0u;
      sb = sb2;
      pd = pd2;
    }
    nu += ((sb | pd) >> key) & 1u;
    np += (pd >> key) & 1u;
  }
  if (nu) atomicAdd(&s_n[0], nu);
  if (np) atomicAdd(&s_n[1], np);
  if (nc) atomicAdd(&s_n[2], nc);
  __syncthreads();
  if (tid == 0) {
    *LD.cnt_u(key, b) = s_n[0];
    *LD.cnt_p(key, b) = s_n[1];
    if (s_n[2]) atomicAdd(LD.ctr(kLsSubscribes), (unsigned long long)s_n[2]);
  }
}

void launch_listing_plan(agx_engine* e, uint32_t* blc, uint32_t replan) {
  hipLaunchKernelGGL(k_listing_plan, dim3(1), dim3(kTpThreads), 0, e->stream, e->d_recep, blc, replan);
}

agx_status launch_apply(agx_engine* e, const DevMsgs& sorted) {
  // the chunk histograms consumed by this step's first pass were zeroed by k_chunk_downsweep;
  // on the multi-rank path (no chunk pass) they are never read, so stale columns are harmless
  BucketArgs ba{};
  ba.P = make_params(e);
  ba.in = sorted.c();
  ba.d_n = e->d_n;
  ba.bstart = e->d_bstart;
  ba.scr = e->scr.m();
  ba.bl = e->bl.m();
  ba.em = e->em.m();
  ba.chunk_off = e->d_chunk_off;
  ba.chunk_cnt = e->d_chunk_cnt;
  ba.nhist = e->d_hist_c;
  ba.nhist_stride = e->cstride;
  ba.G = e->G;
  ba.ng = e->ng;
  ba.nx_shift = e->plan.shift[0];
  ba.nx_bits = e->plan.bits[0];
  ba.nb = e->nb;
  ba.bb = e->bb;
  ba.kmax = e->kmax;
  ba.stats = e->d_stats;
  ba.bstats = e->d_bstats;
  ba.skew_list = e->d_skew_list;
  ba.skew_n = e->d_skew_n;
  if (e->fused) {
    ba.par = e->par;
    ba.slot = e->cur_slot;
    if (e->strict_cap) ba.abort = e->d_abort;
    ba.P.step = e->d_parv + e->par;  // CRDT heap parity = superstep parity
  }
  if (e->fused) {
    GatherArgs& g = ba.g;
    g.bl[0] = e->bl.m();
    g.bl[1] = e->bl2.m();
    g.eg[0] = e->eg0.m();
    g.eg[1] = e->eg1.m();
    g.stg = e->stg.c();
    for (int q = 0; q < 2; ++q) {
      g.tcnt[q] = e->d_tcnt[q];
      g.toff[q] = e->d_toff[q];
      g.blo[q] = e->d_blo[q];
      g.blc[q] = e->d_blc[q];
      g.emc[q] = e->d_emc[q];
    }
    g.stg_off = e->d_stg_off;
    g.stg_cnt = e->d_stg_cnt;
    g.inb = e->A.m();
    g.ovf = e->d_ovf;
    g.cntb = e->d_cntb;
    g.heap_top = e->pw ? e->d_heap_top : nullptr;
    g.cap = e->acap;
    g.tstride = e->tstride;
    g.region = e->region;
  }
  if (!e->fused && e->R == 1) {  // multi-pass: the backlog stays in place (parity arenas bl / bl2)
    ba.em = em_arena(e, e->par).m();  // (tells by superstep parity: identity grouping reads the other one)
    if (e->ident_on) {
      ba.ident = e->d_ident;
      ba.in_alt = em_arena(e, e->par ^ 1u).c();
      ba.emmeta = e->d_emmeta;
    }
    ba.pstep = e->d_step;
    ba.cap = e->cap;
    ba.blpre = e->d_blpre;
    ba.bl_sbase = e->d_blpre + e->nb + kMaxBlSlices;
    ba.d_ninbox = e->d_ninbox;
    ba.g.bl[0] = e->bl.m();
    ba.g.bl[1] = e->bl2.m();
  }
  if (e->R > 1) {  // tells leave grouped by owner rank (phase 1 packs them for the exchange)
    ba.nx_shift = kOwnerShift;
    ba.nx_bits = std::max<uint32_t>(1, ceil_log2(e->R));
    ba.g.eg[0] = e->eg0.m();
    ba.g.tcnt[0] = e->d_tcnt[0];
    ba.g.toff[0] = e->d_toff[0];
    ba.g.tstride = e->tstride;
  }
  ba.dbg = e->d_dbg;
  ba.halt = e->R > 1 ? e->d_halt : nullptr;
  ba.tiny_max = e->tiny_max;
  ba.sk_rec = e->d_sk_rec;
  ba.sk_act = e->d_sk_act;
  if (e->ring_live) {
    ba.ring_of = e->d_ring_of;
    ba.ring_state = e->d_ring_state;
    ba.ring_src = e->d_ring_src;
    ba.ring_pay = e->d_ring_pay;
    ba.ring_next = e->d_ring_next;
    ba.ring_free = e->d_ring_free;
    ba.ring_total = e->d_ring_total;
    ba.ring_slots = e->ring_slots;
    ba.ring_c = e->ring_c;
    ba.ring_t = e->Traw;
    ba.ring_lo0 = (uint32_t)e->acap;
  }
  SkewArgs ska{e->d_sk_rec, e->d_sk_act, e->d_sk_pc, e->d_sk_meta, e->sk_budget, e->sk_rows};
  if (e->rg_on) {  // ring apply: one launch does admission, drains and ring appends (agx_ring.h)
    RingArgs ra{e->d_rg_state, e->d_rg_src, e->d_rg_pay, e->d_rg_dk, e->d_rg_ds, e->d_rg_dp, e->d_ring_total,
                e->d_rg_nz, e->rg_c, e->rg_dstride};
    const uint32_t vid = apply_variant(e);
    if (e->tiny_launch && e->tiny_max && !e->skew_only) {  // sparse buckets a wave each, then the marked ones
      ba.blist = e->d_blist;
      Scope s(e, K_TINY);
      HIP_TRY(agx_launch_ring(vid, true, dim3(grid_for((e->nb + kTinyWaves - 1) / kTinyWaves, kMaxApplyGrid)), e->stream,
                              ba, ra));
    }
    {
      Scope s(e, K_RINGAPPLY);
      HIP_TRY(agx_launch_ring(vid, false, dim3(grid_for(e->nb, e->apply_grid)), e->stream, ba, ra));
    }
    e->par ^= 1u;
    HIP_TRY(hipGetLastError());
    return AGX_OK;
  }
  {
    const uint32_t vid = apply_variant(e);
    const bool lwd = vid == V_LWWMAP_DELTA;  // LWWMap with delta replication: state effects in k_lwwmap_delta_merge
    const bool lwm = vid == V_LWWMAP || lwd;  // LWWMap-only: state effects in k_lwwmap_merge
    const bool pnm = vid == V_PNCMAP;       // PNCounterMap-only: state effects in k_pncmap_merge
    const bool mmm = vid == V_ORMM;         // ORMultiMap-only: state effects in k_ormm_merge
    const bool orm = vid == V_OR || lwm || pnm || mmm;  // ORSet-only full state: state effects in k_orset_merge
    if (orm) {
      if (!e->d_orw || (lwm && !e->d_lww_step0)) return set_err(AGX_ESTATE, "ORSet work list not allocated (setup_orset)");
      ba.orw = e->d_orw;
      ba.orm = e->d_orm;
      ba.orw_n = e->d_orw_n;
      HIP_TRY(hipMemsetAsync(e->d_orw_n, 0, 8, e->stream));
    }
    const uint32_t mode = e->fused ? M_FUSED : e->R > 1 ? M_OWNER : M_BYPASS;
    const dim3 g(grid_for(e->nb, e->apply_grid));
    // dense buckets (one message per actor) first, in their own lean launch (k_dense_apply; fused
    // superstep: k_dense_fused); by default for ring populations, whose buckets all are
    // (AGX_DENSE_LAUNCH=1 / 0 forces it; AGX_DENSE_FUSED=0 keeps the fused superstep one launch)
    const bool dl = dense_on(e, vid) && !e->skew_only && !e->recover_dense;
    // fused strict replay: the dense launch alone is the superstep (a bucket it cannot take marks the
    // replay void from there, as a deferred skewed bucket does; run_single recovers it), until the
    // first such recovery (e->dense_alone cleared for the engine)
    const bool alone = dl && mode == M_FUSED && e->strict_cap && e->dense_alone;
    if (dl || e->recover_dense) {
      ba.blist = e->d_blist;
      // (owner mode: one word, [0] -- cleared by the superstep's k_mcompact_scan, before the dense launch)
      ba.dense_left = e->d_dense_left;
    }
    const bool persist = dl && alone && e->persist_steps > 0;
    if (dl) {
      Scope s(e, K_DENSE);
      BucketArgs bd = ba;
      bd.dense_alone = alone ? 1u : 0u;
      if (persist) {  // e->persist_steps supersteps in one launch, one block per bucket (persist_ok)
        bd.psteps = e->persist_steps;
        bd.pbar = e->d_pbar;
        if (bd.par) {  // the kernel's pointer arrays by LOGICAL parity: index 0 = the first superstep's write parity
          GatherArgs& q = bd.g;
          std::swap(q.bl[0], q.bl[1]);
          std::swap(q.eg[0], q.eg[1]);
          std::swap(q.tcnt[0], q.tcnt[1]);
          std::swap(q.toff[0], q.toff[1]);
          std::swap(q.blo[0], q.blo[1]);
          std::swap(q.blc[0], q.blc[1]);
          std::swap(q.emc[0], q.emc[1]);
        }
        HIP_TRY(agx_launch_dense(vid, M_PERSIST, dim3(e->nb), e->stream, bd));
      } else {
        HIP_TRY(agx_launch_dense(vid, mode, dim3(grid_for(e->nb, kMaxApplyGrid)), e->stream, bd));
      }
    }
    if (dl && e->prof && !persist && mode != M_OWNER) {
      // (profiling only: eager launches) the launch cleared the other parity's word and raised this
      // one's iff it left a bucket, so both words zero = it took every bucket and the wave / block
      // launches below return at entry (bench.py marks them returned_at_entry from this count)
      uint32_t w2[2] = {1u, 1u};
      HIP_TRY(hipMemcpyAsync(w2, e->d_dense_left, 8, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      if (w2[0] == 0u && w2[1] == 0u) ++e->prof_items[K_DENSE];
    }
    if (persist) {  // (nothing else runs in a dense-alone strict superstep)
      if (e->persist_steps & 1u) e->par ^= 1u;
      HIP_TRY(hipGetLastError());
      return AGX_OK;
    }
    // (priority mailboxes: the wave path drains in arrival order -- every bucket takes the block launch)
    const bool tl = mode == M_BYPASS && !kVariants[vid].wide && e->tiny_launch && e->tiny_max && !e->skew_only &&
                    active_feature(e) == F_NONE;
    if (tl) {  // wave-per-bucket launch first; the block launch then takes the buckets it marked
      ba.blist = e->d_blist;
      ba.dense_first = dl ? 1u : 0u;
      Scope s(e, K_TINY);
      const uint32_t gt = grid_for((e->nb + kTinyWaves - 1) / kTinyWaves, kMaxApplyGrid);
      HIP_TRY(agx_launch_tiny(vid, dim3(gt), e->stream, ba));
    }
    // skew list (grid-stride); ring buckets take the skew launch every superstep: a wider grid then
    const dim3 gs(grid_for(e->nb, std::min(e->apply_grid, e->ring_live ? std::max(e->skew_grid, 2048u) : e->skew_grid)));
    if (!e->skew_only && !alone) {
      Scope s(e, K_APPLY);
      BucketArgs bf = ba;
      if (e->stamps_skew) bf.dbg = nullptr;  // (diagnostic: stamps of the skew launch only)
      if (const Feature a = active_feature(e); a != F_NONE) {
        if (mode == M_OWNER) return set_err(AGX_ESTATE, "%s a single-rank engine", kFeatures[a].needs);
        const FeatureRow& F = kFeatures[launched_feature(e, a)];
        HIP_TRY(agx_launch_apply_feature(vid, mode, F.km, F.prio, g, e->stream, bf));
      } else {
        HIP_TRY(agx_launch_apply(vid, mode, false, g, e->stream, bf));
      }
    }
    if (!(mode == M_FUSED && e->strict_cap)) {
      if (!kVariants[vid].wide && mode == M_BYPASS) {
        Scope s(e, K_SKEWPRE);  // (k_skew_plan / count / scan / scatter: their own profiling class)
        skew_prepass(e, ba, ska);
      }
      Scope s(e, K_SKEW);
      HIP_TRY(agx_launch_apply(vid, mode, true, gs, e->stream, ba));
    }
    if (lwd) {
      Scope s(e, K_APPLY);
      HIP_TRY(agx_launch_lwwmap_delta_merge(dim3(grid_for(e->n_local / 4 + 1, 4096)), e->stream, ba.P, (const uint4*)e->d_orw,
                                            (const uint2*)e->d_orm, (const uint32_t*)e->d_orw_n, e->d_lww_step0, e->cur_slot,
                                            e->lww_clock, (int64_t)e->lww_base));
    } else if (lwm) {
      Scope s(e, K_APPLY);
      HIP_TRY(agx_launch_lwwmap_merge(dim3(grid_for(e->n_local / 4 + 1, 4096)), e->stream, ba.P, (const uint4*)e->d_orw,
                                      (const uint2*)e->d_orm, (const uint32_t*)e->d_orw_n, e->d_lww_step0, e->cur_slot,
                                      e->lww_clock, (int64_t)e->lww_base));
    } else if (pnm) {
      Scope s(e, K_APPLY);
      HIP_TRY(agx_launch_pncmap_merge(dim3(grid_for(e->n_local / 4 + 1, 4096)), e->stream, ba.P, (const uint4*)e->d_orw,
                                      (const uint2*)e->d_orm, (const uint32_t*)e->d_orw_n));
    } else if (mmm) {
      Scope s(e, K_APPLY);
      HIP_TRY(agx_launch_ormm_merge(dim3(grid_for(e->n_local / 4 + 1, 4096)), e->stream, ba.P, (const uint4*)e->d_orw,
                                    (const uint2*)e->d_orm, (const uint32_t*)e->d_orw_n));
    } else if (orm) {
      Scope s(e, K_APPLY);
      hipLaunchKernelGGL(k_orset_merge, dim3(grid_for(e->n_local / 4 + 1, 4096)), dim3(kThreads), 0, e->stream, ba.P,
                         (const uint4*)e->d_orw, (const uint2*)e->d_orm, (const uint32_t*)e->d_orw_n);
    }
  }
  if (e->d_recep) launch_recep_rebuild(e);  // (every superstep, captured or eager: the listings of the next tick)
  // (... and the tick's publications: the backlog counts this superstep wrote carry the next tick's deliveries)
  if (e->d_topic) launch_topic_plan(e, e->fused ? e->d_blc[e->par] : e->d_chunk_cnt, 0u);
  if (e->d_list) launch_listing_plan(e, e->fused ? e->d_blc[e->par] : e->d_chunk_cnt, 0u);  // (... and the owed Listings)
  if (e->R == 1) e->par ^= 1u;  // the next superstep writes the other parity (fused and multi-pass)
  HIP_TRY(hipGetLastError());
  return AGX_OK;
}

// host-staged tells enter as chunk 2nb of the next single-rank step
agx_status launch_staged_chunk(agx_engine* e) {
  if (!e->n_staged_dev) return AGX_OK;
  hipLaunchKernelGGL(k_chunk_hist, dim3(kStagedChunks), dim3(kThreads), 0, e->stream, e->stg.key, e->n_staged_dev,
                     e->d_hist_c, e->cstride, 2 * e->ng, e->plan.shift[0], e->plan.bits[0], e->d_chunk_off,
                     e->d_chunk_cnt, 2 * e->nb);
  HIP_TRY(hipGetLastError());
  e->n_staged_dev = 0;
  return AGX_OK;
}

// Bounded-mailbox rings: allocate the pool at the first run whose configuration allows it (plain
// behaviours, every configured mailbox class bounded by <= kRingMaxC); from then on the classes
// are fixed (agx_set_mailbox_class refuses a capacity the rings cannot hold).
agx_status setup_rings(agx_engine* e) {
  if (e->ring_live || !e->ring_res || e->pw || active_feature(e) != F_NONE) return AGX_OK;  // (a ring drains in arrival order)
  uint32_t cmax = 0;
  for (uint32_t c = 0; c < AGX_MAX_MAILBOX_CLASSES; ++c) {
    if (!((e->mclass_set >> c) & 1u)) continue;
    if (e->mcap[c] == 0 || e->mcap[c] > kRingMaxC) return AGX_OK;  // an unbounded (or large) mailbox class
    cmax = std::max(cmax, e->mcap[c]);
  }
  uint64_t budget = kRingPoolBytes;
  if (const char* s = getenv("AGX_RING_MB")) budget = (uint64_t)std::max(0, atoi(s)) << 20;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::min<uint64_t>(budget, fr / 4);
  const uint64_t per = (uint64_t)kBucket * (2ull * cmax + 1) * 4;
  const uint32_t slots = (uint32_t)std::min<uint64_t>(e->ring_res, budget / per);
  if (!slots) return AGX_OK;
  const uint64_t nst = (uint64_t)slots * kBucket, nmsg = nst * cmax;
  AGX_TRY(dalloc(&e->d_ring_of, e->nb));
  AGX_TRY(dalloc(&e->d_ring_state, nst));
  AGX_TRY(dalloc(&e->d_ring_src, nmsg));
  AGX_TRY(dalloc(&e->d_ring_pay, nmsg));
  AGX_TRY(dalloc(&e->d_ring_next, 2));
  AGX_TRY(dalloc(&e->d_ring_free, slots));
  AGX_TRY(dalloc(&e->d_ring_total, 2));
  HIP_TRY(hipMemsetAsync(e->d_ring_of, 0, e->nb * 4ull, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_ring_state, 0, nst * 4, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_ring_next, 0, 8, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_ring_total, 0, 8, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ring_slots = slots;
  e->ring_c = cmax;
  e->ring_live = true;
  drop_graphs(e);  // the ring arrays are kernel arguments of the captured supersteps
  return AGX_OK;
}

// Ring apply (agx_ring.h), decided once before the first superstep: a single-rank multi-pass engine
// with plain behaviours, one tell per message (max_emit 1) and every mailbox class bounded keeps its
// queued messages in per-actor rings of the largest capacity when they fit the HBM budget (at most
// half of the free memory: n_local x capacity x 8 B, C5's 10^8 actors x 64 = 51 GB of a 288 GB
// MI355X), so a queued message is written once and read once instead of being copied forward by every
// superstep it waits.  Each bucket's tells get a fixed slice of kBucket x throughput slots of the tell
// arenas (a bucket may drain more messages than it receives: its rings' heads).
constexpr uint32_t kRingAutoC = 256;  // ring apply by default from this mailbox capacity up (setup_ring_apply)
agx_status setup_ring_apply(agx_engine* e) {
  if (e->started || e->rg_on || e->ring_live || e->ring_res) return AGX_OK;
  if (e->fused || e->R != 1 || e->pw || e->kmax != 1 || e->n_local == 0 || active_feature(e) != F_NONE) return AGX_OK;
  // AGX_RING_APPLY=1 / 0 forces rings on / off; unset: on when the largest bounded capacity is at
  // least kRingAutoC.  Deep queues are where re-copying the backlog every superstep costs most (C3,
  // BoundedMailbox(1000): 4.67e8 -> 6.7e8 msg/s with rings, the sparse buckets a wave each); at
  // C5's BoundedMailbox(64) the hub buckets' serial ring chain in one block still loses (2.9e9 with
  // the backlog arena vs 1.8e9).
  const char* rs = getenv("AGX_RING_APPLY");
  const int force = rs ? atoi(rs) : -1;
  if (force == 0) return AGX_OK;
  if (kVariants[apply_variant(e)].wide) return AGX_OK;
  uint32_t cmax = 0;
  for (uint32_t c = 0; c < AGX_MAX_MAILBOX_CLASSES; ++c) {
    if (!((e->mclass_set >> c) & 1u)) continue;
    if (e->mcap[c] == 0 || e->mcap[c] > kRingApplyMaxC) return AGX_OK;  // an unbounded (or huge) mailbox class
    cmax = std::max(cmax, e->mcap[c]);
  }
  if (force < 0 && cmax < kRingAutoC) return AGX_OK;
  const uint64_t dstr = e->Traw, slice = (uint64_t)kBucket * dstr;  // (drained per actor <= min(T, C) <= Traw)
  const uint64_t em_need = (uint64_t)e->nb * slice;
  if (em_need >= (1ull << 32)) return AGX_OK;
  const uint64_t ring_bytes = e->n_local * (uint64_t)cmax * 8 + e->n_local * 4;
  const uint64_t scratch_bytes = em_need * 12;
  const uint64_t em_bytes = em_need > e->em_cap ? 2 * em_need * 12 : 0;  // (bigger tell arenas, both parities)
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return AGX_OK;
  if (ring_bytes + scratch_bytes + em_bytes > fr / 2) return AGX_OK;  // the backlog arena, as before
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (em_need > e->em_cap) {
    free_msgs(e->em);
    free_msgs(e->em2);
    AGX_TRY(alloc_msgs(e->em, em_need));
    AGX_TRY(alloc_msgs(e->em2, em_need));
    e->em_cap = em_need;
  }
  AGX_TRY(dalloc(&e->d_rg_state, e->n_local));
  AGX_TRY(dalloc(&e->d_rg_nz, (uint64_t)e->nb * (kBucket / 32)));
  AGX_TRY(dalloc(&e->d_rg_src, e->n_local * (uint64_t)cmax));
  AGX_TRY(dalloc(&e->d_rg_pay, e->n_local * (uint64_t)cmax));
  AGX_TRY(dalloc(&e->d_rg_dk, em_need));
  AGX_TRY(dalloc(&e->d_rg_ds, em_need));
  AGX_TRY(dalloc(&e->d_rg_dp, em_need));
  if (!e->d_ring_total) AGX_TRY(dalloc(&e->d_ring_total, 2));
  HIP_TRY(hipMemsetAsync(e->d_rg_state, 0, e->n_local * 4, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_rg_nz, 0, (size_t)e->nb * (kBucket / 32) * 4, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_ring_total, 0, 16, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->rg_c = cmax;
  e->rg_dstride = (uint32_t)dstr;
  e->rg_on = true;
  drop_graphs(e);  // the arenas are kernel arguments of the captured supersteps
  return AGX_OK;
}

// ORSet-only full-state populations: k_orset_merge's work list (before any graph capture)
agx_status setup_orset(agx_engine* e) {
  const uint32_t vid = apply_variant(e);
  if (e->d_orw || (vid != V_OR && vid != V_LWWMAP && vid != V_PNCMAP && vid != V_ORMM && vid != V_LWWMAP_DELTA)) return AGX_OK;
  if (vid == V_LWWMAP || vid == V_LWWMAP_DELTA) {
    AGX_TRY(dalloc(&e->d_lww_step0, 1));
    HIP_TRY(hipMemset(e->d_lww_step0, 0, 4));
  }
  AGX_TRY(dalloc(&e->d_orw, e->n_local));
  AGX_TRY(dalloc(&e->d_orm, e->acap));
  AGX_TRY(dalloc(&e->d_orw_n, 2));
  return AGX_OK;
}

agx_status copy_sync(agx_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

// the drain limit of mailbox class c (mbox_limits on the device)
uint32_t class_throughput(const agx_engine* e, uint32_t c) {
  if (!e->mclasses) return std::max<uint32_t>(e->T, 1u);
  const uint32_t C = e->mcap[c], T = std::max<uint32_t>(e->Traw, 1u);
  return C && T > C ? C : T;
}

// Deque-based mailboxes (agx_set_stash): the stash storage (agx_device.h StashDev) -- allocated and
// zeroed once, sized by n_local: every actor has a header, Smax buffer slots and Pmax park slots, so an
// actor's slot needs no indirection and a class can be bound to any actor later; then the classes'
// capacities and the marks of the buckets that hold an actor of a stash class.
agx_status upload_stash(agx_engine* e) {
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  if (!e->d_stash) {
    uint32_t smax = 1, tmax = 1;
    for (uint32_t c = 0; c < AGX_MAX_MAILBOX_CLASSES; ++c) {
      if (!((e->mclass_set >> c) & 1u)) continue;
      smax = std::max(smax, e->stash_cap[c]);
      tmax = std::max(tmax, class_throughput(e, c));
    }
    const uint32_t pmax = std::min<uint32_t>(tmax - 1u, (uint32_t)kBucket - 1u);  // (a park is the rest of one drain window)
    const uint64_t hoff = ((uint64_t)kStashBucketOff + 2ull * e->nb + 1ull) & ~1ull;
    const uint64_t soff = hoff + 2ull * npad;
    const uint64_t total = soff + 2ull * npad * ((uint64_t)smax + pmax);
    if (hipMalloc((void**)&e->d_stash, total * 4ull) != hipSuccess) {
      (void)hipGetLastError();
      e->d_stash = nullptr;
      return set_err(AGX_ENOMEM, "the stash buffers of %llu actors (%u buffer + %u park envelopes each, %llu MB) do not "
                     "fit on the device", (unsigned long long)npad, smax, pmax, (unsigned long long)(total >> 18));
    }
    // (headers, pending counts and counters start at zero; the envelopes need no initial value)
    HIP_TRY(hipMemsetAsync(e->d_stash, 0, soff * 4ull, e->stream));
    e->stash_smax = smax;
    e->stash_pmax = pmax;
    e->stash_hdr_off = hoff;
    e->stash_slot_off = soff;
    drop_graphs(e);  // (a kernel argument of the captured supersteps)
  }
  uint32_t head[16] = {0};
  for (uint32_t c = 0; c < AGX_MAX_MAILBOX_CLASSES; ++c) head[c] = e->stash_cap[c];
  head[8] = e->stash_smax;
  head[9] = e->stash_pmax;
  std::vector<uint32_t> marks(e->nb, 0);
  for (uint64_t l = 0; l < e->n_local; ++l)
    if (e->stash_cap[(e->h_alive[l] >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1)]) marks[l >> e->bb] = 1;
  HIP_TRY(hipMemcpyAsync(e->d_stash, head, sizeof(head), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_stash + kStashBucketOff + e->nb, marks.data(), marks.size() * 4ull, hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->stash_dirty = false;
  return AGX_OK;
}

// The stash headers of every actor, read back: buffered messages not released (held), released or
// parked ones still to be processed (pending), and how many of the pending ones the buckets' backlog
// counts already carry (the next superstep's windows: counted by the device's in-flight sum).
agx_status stash_scan(agx_engine* e, uint64_t* held, uint64_t* pending, uint64_t* windows) {
  *held = *pending = *windows = 0;
  if (!e->d_stash) return AGX_OK;
  std::vector<uint32_t> h(2ull * e->n_local);
  AGX_TRY(copy_sync(e, h.data(), e->d_stash + e->stash_hdr_off, h.size() * 4ull, hipMemcpyDeviceToHost));
  for (uint64_t l = 0; l < e->n_local; ++l) {
    const uint32_t x = h[2 * l], y = h[2 * l + 1];
    const uint32_t rel = (x >> 8) & 0xFFu, size = (x >> 16) & 0xFFu, pc = y >> 16;
    if (!size && !pc) continue;
    const uint32_t T = class_throughput(e, (e->h_alive[l] >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1));
    *held += size - rel;
    *pending += rel + pc;
    *windows += rel ? std::min(rel, T) : std::min(pc, T);
  }
  return AGX_OK;
}

// ---- timers (agx_set_timers)
// agx_start_timers on the device: one thread per actor of the range starts slot `key` at its bucket's clock
static __global__ void __launch_bounds__(kThreads) k_timer_start(uint32_t* tm, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                                uint32_t first, uint32_t count, uint32_t key, uint32_t periodic,
                                                                uint32_t delay, const uint32_t* delays, uint32_t payload) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const uint32_t l = first + i, np = nb << bb;
  if (!(alive[l] & 1u)) return;  // (a stopped actor has no timers)
  const uint32_t nk = tm[0];
  uint32_t* const next = tm + tm_slot_off(nb);
  uint32_t *const per = next + (size_t)nk * np, *const gen = per + (size_t)nk * np, *const pay = gen + (size_t)nk * np,
           *const agen = pay + (size_t)nk * np;
  // the first fire after delays[i] ticks (`delay` without the array); a periodic timer's period is `delay`
  auto clamp = [](uint32_t x) { return x < 1u ? 1u : x > kTmMaxDelay ? kTmMaxDelay : x; };
  const uint32_t d = clamp(delays ? delays[i] : delay), pd = clamp(delay);
  const size_t x = (size_t)key * np + l;
  const uint32_t g = agen[l] + 1u;
  agen[l] = g;
  gen[x] = g;
  pay[x] = payload;
  per[x] = (periodic ? pd : 0u) | kTmActive;
  next[x] = tm[kTmBucketOff + 2u * nb + (l >> bb)] + d;
}
// after host-side starts: every bucket's earliest fire and the fires of its next tick, whose count replaces
// the old one in the bucket's backlog count (one block per bucket)
static __global__ void __launch_bounds__(kThreads) k_timer_sync(uint32_t* tm, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                               uint32_t n_local, uint32_t* blc) {
  __shared__ uint32_t s_min, s_due;
  const uint32_t b = blockIdx.x, np = nb << bb, nk = tm[0];
  if (threadIdx.x == 0) {
    s_min = kTmNone;
    s_due = 0u;
  }
  __syncthreads();
  const uint32_t* next = tm + tm_slot_off(nb);
  const uint32_t now = tm[kTmBucketOff + 2u * nb + b];
  const uint32_t a0 = b << bb, na = min(1u << bb, n_local - a0);
  uint32_t mn = kTmNone, nd = 0;
  for (uint32_t k = 0; k < nk; ++k)
    for (uint32_t la = threadIdx.x; la < na; la += kThreads) {
      const uint32_t n = next[(size_t)k * np + a0 + la];
      if (n != kTmNone && (alive[a0 + la] & 1u)) {
        mn = min(mn, n);
        nd += n == now + 1u ? 1u : 0u;
      }
    }
  if (mn != kTmNone) atomicMin(&s_min, mn);
  if (nd) atomicAdd(&s_due, nd);
  __syncthreads();
  if (threadIdx.x == 0) {
    tm[kTmBucketOff + b] = s_min;
    blc[b] = blc[b] - min(tm[kTmBucketOff + nb + b], blc[b]) + s_due;
    tm[kTmBucketOff + nb + b] = s_due;
  }
}

// ---- receive timeouts (agx_set_receive_timeout): the rows after the timers' (agx_device.h IdleDev)
// agx_start_receive_timeout on the device: one thread per actor of the range sets (delay, payload) at its bucket's
// clock; delay 0 cancels
static __global__ void __launch_bounds__(kThreads) k_rt_start(uint32_t* tm, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                             uint32_t first, uint32_t count, uint32_t delay, uint32_t payload) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const uint32_t l = first + i, np = nb << bb;
  if (!(alive[l] & 1u)) return;  // (a stopped actor has no timeout)
  uint32_t* const rnext = tm + tm_slot_off(nb) + (4ull * tm[0] + 1ull) * np;
  const uint32_t d = delay > kTmMaxDelay ? kTmMaxDelay : delay;
  rnext[l] = d ? tm[kTmBucketOff + 2u * nb + (l >> bb)] + d : kTmNone;
  rnext[(size_t)np + l] = d;
  if (d) rnext[2ull * np + l] = payload;
}
// k_timer_sync of an engine with receive timeouts: the idle row counts as one more key
static __global__ void __launch_bounds__(kThreads) k_rt_sync(uint32_t* tm, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                            uint32_t n_local, uint32_t* blc) {
  __shared__ uint32_t s_min, s_due;
  const uint32_t b = blockIdx.x, np = nb << bb, nk = tm[0];
  if (threadIdx.x == 0) {
    s_min = kTmNone;
    s_due = 0u;
  }
  __syncthreads();
  const uint32_t* next = tm + tm_slot_off(nb);
  const uint32_t* rnext = next + (4ull * nk + 1ull) * np;
  const uint32_t now = tm[kTmBucketOff + 2u * nb + b];
  const uint32_t a0 = b << bb, na = min(1u << bb, n_local - a0);
  uint32_t mn = kTmNone, nd = 0;
  for (uint32_t k = 0; k <= nk; ++k)
    for (uint32_t la = threadIdx.x; la < na; la += kThreads) {
      const uint32_t n = k < nk ? next[(size_t)k * np + a0 + la] : rnext[a0 + la];
      if (n != kTmNone && (alive[a0 + la] & 1u)) {
        mn = min(mn, n);
        nd += n == now + 1u ? 1u : 0u;
      }
    }
  if (mn != kTmNone) atomicMin(&s_min, mn);
  if (nd) atomicAdd(&s_due, nd);
  __syncthreads();
  if (threadIdx.x == 0) {
    tm[kTmBucketOff + b] = s_min;
    blc[b] = blc[b] - min(tm[kTmBucketOff + nb + b], blc[b]) + s_due;
    tm[kTmBucketOff + nb + b] = s_due;
  }
}

// ---- the ask pattern (agx_set_ask): the row after the timers' (agx_device.h AskDev)
// after agx_start_timers on an engine with ask: the started slots hold plain timers, no ask's timeout
static __global__ void __launch_bounds__(kThreads) k_ask_clear(uint32_t* tm, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                              uint32_t first, uint32_t count, uint32_t key) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const uint32_t l = first + i, np = nb << bb;
  if (!(alive[l] & 1u)) return;  // (k_timer_start left a stopped actor's slot alone)
  uint32_t* const row = tm + tm_slot_off(nb) + (4ull * tm[0] + 1ull) * np;
  row[(size_t)key * np + l] = 0u;
}

size_t timers_words(const agx_engine* e) {
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  return tm_slot_off(e->nb) + (4ull * e->tm_keys + 1ull) * npad + (e->rt_on ? 3ull * npad + 8ull : 0ull) +
         (e->ask_on ? (uint64_t)e->tm_keys * npad : 0ull);
}
// the receive-timeout rows of the timer storage: rt_next, then rt_delay, rt_pay and the mask (agx_device.h IdleDev)
size_t rt_row_off(const agx_engine* e) {
  return tm_slot_off(e->nb) + (4ull * e->tm_keys + 1ull) * ((uint64_t)e->nb << e->bb);
}

// the ask row of the timer storage, [key][actor] (agx_device.h AskDev; an engine has receive timeouts or ask, not both)
size_t ask_row_off(const agx_engine* e) { return rt_row_off(e); }

// The timer storage (agx_device.h TimerDev) -- allocated once, sized by n_local: counters, clocks and due counts
// zero, every bucket's earliest fire and every slot's next fire "none", the slots inactive.
agx_status alloc_timers(agx_engine* e) {
  if (e->d_timers) return AGX_OK;
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  const size_t total = timers_words(e), soff = tm_slot_off(e->nb);
  if (hipMalloc((void**)&e->d_timers, total * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_timers = nullptr;
    return set_err(AGX_ENOMEM, "the timer slots of %llu actors (%u keys each, %llu MB) do not fit on the device",
                   (unsigned long long)npad, e->tm_keys, (unsigned long long)(total >> 18));
  }
  HIP_TRY(hipMemsetAsync(e->d_timers, 0, total * 4ull, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_timers + kTmBucketOff, 0xFF, (size_t)e->nb * 4ull, e->stream));       // earliest
  HIP_TRY(hipMemsetAsync(e->d_timers + soff, 0xFF, (size_t)e->tm_keys * npad * 4ull, e->stream));  // next
  if (e->rt_on) {
    HIP_TRY(hipMemsetAsync(e->d_timers + rt_row_off(e), 0xFF, npad * 4ull, e->stream));  // rt_next
    HIP_TRY(hipMemcpyAsync(e->d_timers + rt_row_off(e) + 3ull * npad, e->rt_mask, sizeof(e->rt_mask), hipMemcpyHostToDevice,
                           e->stream));
  }
  const uint32_t nk = e->tm_keys;
  HIP_TRY(hipMemcpyAsync(e->d_timers, &nk, 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  drop_graphs(e);  // (a kernel argument of the captured supersteps)
  return AGX_OK;
}

// the backlog counts the next superstep reads (fused: the read parity's; multi-pass: the chunk counts)
uint32_t* next_backlog_counts(agx_engine* e) { return e->fused ? e->d_blc[e->par ^ 1u] : e->d_chunk_cnt; }

// apply the recorded agx_start_timers calls (the actors' flags are on the device: prepare_run)
agx_status flush_timer_starts(agx_engine* e) {
  if (e->tm_starts.empty() && e->rt_starts.empty()) return AGX_OK;
  if (e->actors_dirty)  // (a query before the run: the host's flags are the newer ones; prepare_run uploads the rest)
    HIP_TRY(hipMemcpyAsync(e->d_alive, e->h_alive.data(), e->n_local, hipMemcpyHostToDevice, e->stream));
  for (const auto& ts : e->tm_starts) {
    uint32_t* d_del = nullptr;
    if (!ts.delays.empty()) {
      AGX_TRY(dalloc(&d_del, ts.delays.size()));
      HIP_TRY(hipMemcpyAsync(d_del, ts.delays.data(), ts.delays.size() * 4ull, hipMemcpyHostToDevice, e->stream));
    }
    if (ts.count)
      hipLaunchKernelGGL(k_timer_start, dim3((uint32_t)((ts.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, e->stream,
                         e->d_timers, e->d_alive, e->nb, e->bb, (uint32_t)ts.first, (uint32_t)ts.count, ts.key, ts.periodic,
                         ts.delay, d_del, ts.payload);
    if (ts.count && e->ask_on)
      hipLaunchKernelGGL(k_ask_clear, dim3((uint32_t)((ts.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, e->stream,
                         e->d_timers, e->d_alive, e->nb, e->bb, (uint32_t)ts.first, (uint32_t)ts.count, ts.key);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (d_del) hipFree(d_del);
  }
  e->tm_starts.clear();
  for (const auto& rs : e->rt_starts) {  // (after the timer starts: a call order between the two kinds does not matter)
    if (rs.count)
      hipLaunchKernelGGL(k_rt_start, dim3((uint32_t)((rs.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, e->stream,
                         e->d_timers, e->d_alive, e->nb, e->bb, (uint32_t)rs.first, (uint32_t)rs.count, rs.delay, rs.payload);
    HIP_TRY(hipGetLastError());
  }
  e->rt_starts.clear();
  if (e->rt_on)
    hipLaunchKernelGGL(k_rt_sync, dim3(e->nb), dim3(kThreads), 0, e->stream, e->d_timers, e->d_alive, e->nb, e->bb,
                       (uint32_t)e->n_local, next_backlog_counts(e));
  else
  hipLaunchKernelGGL(k_timer_sync, dim3(e->nb), dim3(kThreads), 0, e->stream, e->d_timers, e->d_alive, e->nb, e->bb,
                     (uint32_t)e->n_local, next_backlog_counts(e));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->inflight_known = false;
  return AGX_OK;
}

// the bookkeeping words of the timer storage: [0, kTmBucketOff) then earliest / due / clock per bucket
agx_status read_timer_head(agx_engine* e, std::vector<uint32_t>& h) {
  h.assign(kTmBucketOff + 3ull * e->nb, 0u);
  return copy_sync(e, h.data(), e->d_timers, h.size() * 4ull, hipMemcpyDeviceToHost);
}

// after a run: the ticks that passed while the engine was not quiescent (the device's last active tick against
// the clock before the run), and the clock now
agx_status timers_after_run(agx_engine* e) {
  if (!e->d_timers) return AGX_OK;
  uint32_t la = 0, clk = 0;
  AGX_TRY(copy_sync(e, &la, e->d_timers + kTmLastAct, 4, hipMemcpyDeviceToHost));
  AGX_TRY(copy_sync(e, &clk, e->d_timers + kTmBucketOff + 2ull * e->nb, 4, hipMemcpyDeviceToHost));
  if (la > e->tm_clock) e->tm_ticks += la - e->tm_clock;
  e->tm_clock = clk;
  return AGX_OK;
}

// ---- death watch (agx_set_death_watch)
// the death ticks follow the actors' flags: an actor that is not alive and has no death tick yet was never
// registered (before the first run: dead before tick 1) or was stopped from the host (dead in the current tick)
// (children: an id of a child block keeps "none" until it was created and stopped on the device)
static __global__ void __launch_bounds__(kThreads) k_watch_died(uint32_t* wd, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                               uint32_t n_local, uint32_t started, uint32_t children) {
  const uint32_t l = blockIdx.x * kThreads + threadIdx.x, np = nb << bb;
  if (l >= np) return;
  uint32_t* const died = wd + wd_slot_off(nb) + 4ull * wd[0] * np;
  if (children && child_dev(wd, nb).parent_of(l) != kWdNone) return;
  if (l >= n_local || !(alive[l] & 1u)) {
    if (died[l] == kWdNone) died[l] = started ? wd[kWdBucketOff + 2u * nb + (l >> bb)] : 0u;
  }
}
// agx_start_watch on the device, first step: one thread per actor of the range records the watch by the rules of
// a device watch.  A conflicting actor stops (in the current tick); `slot_of[i]` is the slot occupied, or none.
static __global__ void __launch_bounds__(kThreads) k_watch_start(uint32_t* wd, uint8_t* alive, uint32_t nb, uint32_t bb,
                                                                uint32_t n, uint32_t first, uint32_t count,
                                                                const uint32_t* watchees, uint32_t offset, uint32_t with,
                                                                uint32_t payload, uint32_t* slot_of) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const WatchDev WD = watch_dev(wd, nb, bb, n);
  const uint32_t l = first + i, b = l >> bb;
  slot_of[i] = WD.ns;
  if (!(alive[l] & 1u) || WD.died[l] != kWdNone) return;  // (a stopped actor watches nothing)
  const uint32_t x = watchees ? watchees[i] : (uint32_t)(((uint64_t)l + offset) % n);
  uint32_t slot = WD.ns;
  if (WD.watch(l, b, x, with != 0u, payload, &slot)) {  // checkWatchingSame: IllegalStateException
    alive[l] &= 0xFEu;
    WD.stop(l, b, WD.clock(b));
    atomicAdd(WD.ctr(kWcConflicts), 1ull);
  } else {
    slot_of[i] = slot;
  }
}
// second step: a slot occupied by this call whose watchee is dead by now is due at once; its count joins the
// bucket's due count and backlog count, so the next tick's inbox has room for the Terminated envelope
static __global__ void __launch_bounds__(kThreads) k_watch_start_due(uint32_t* wd, uint32_t nb, uint32_t bb, uint32_t n,
                                                                    uint32_t first, uint32_t count, const uint32_t* slot_of,
                                                                    uint32_t* blc) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const WatchDev WD = watch_dev(wd, nb, bb, n);
  const uint32_t l = first + i, b = l >> bb, k = slot_of[i];
  if (k >= WD.ns) return;
  const size_t x = WD.at(k, l);
  if ((WD.st[x] & kWdStateMask) != kWdWatching) return;  // (freed again: the actor was stopped by a conflict)
  const uint32_t w = WD.wee[x];
  if (w < n && WD.died[w] == kWdNone) return;
  WD.st[x] = kWdDue | (WD.st[x] & kWdHasMsg);
  atomicSub(WD.nwatch(b), 1u);
  atomicAdd(WD.due(b), 1u);
  atomicAdd(&blc[b], 1u);
}
// third step: a bucket with a watching slot marks the current tick's "a slot is watching" word (the stop rule of
// the next tick's entry reads it)
static __global__ void __launch_bounds__(kThreads) k_watch_start_any(uint32_t* wd, uint32_t nb) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= nb) return;
  if (wd[kWdBucketOff + 3u * nb + b]) {
    const uint32_t clk = wd[kWdBucketOff + 2u * nb + b];
    wd[kWdAnyW + (clk & 1u)] = clk;
  }
}

size_t watch_words(const agx_engine* e) {
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  return wd_slot_off(e->nb) + (4ull * e->wd_slots + 1ull) * npad;
}

// The watch storage (agx_device.h WatchDev) -- allocated once, sized by n_local: everything zero (slots free),
// the stop / watching words and every death tick "none"
agx_status alloc_watch(agx_engine* e) {
  if (e->d_watch) return AGX_OK;
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  const size_t total = watch_words(e);
  if (hipMalloc((void**)&e->d_watch, total * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_watch = nullptr;
    return set_err(AGX_ENOMEM, "the watch slots of %llu actors (%u slots each, %llu MB) do not fit on the device",
                   (unsigned long long)npad, e->wd_slots, (unsigned long long)(total >> 18));
  }
  HIP_TRY(hipMemsetAsync(e->d_watch, 0, total * 4ull, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_watch + kWdStopW, 0xFF, 4ull * 4ull, e->stream));                     // stopw, anyw
  HIP_TRY(hipMemsetAsync(e->d_watch + (total - npad), 0xFF, npad * 4ull, e->stream));               // died
  const uint32_t ns = e->wd_slots;
  HIP_TRY(hipMemcpyAsync(e->d_watch, &ns, 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->wd_died_init = false;
  drop_graphs(e);  // (a kernel argument of the captured supersteps)
  return AGX_OK;
}

// bring the death ticks up to date with the actors' flags (after registrations)
agx_status watch_sync_died(agx_engine* e) {
  if (e->wd_died_init) return AGX_OK;
  if (e->actors_dirty)  // (a query before the run: the host's flags are the newer ones; prepare_run uploads the rest)
    HIP_TRY(hipMemcpyAsync(e->d_alive, e->h_alive.data(), e->n_local, hipMemcpyHostToDevice, e->stream));
  const uint32_t np = e->nb << e->bb;
  hipLaunchKernelGGL(k_watch_died, dim3((np + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream, e->d_watch, e->d_alive,
                     e->nb, e->bb, (uint32_t)e->n_local, e->started ? 1u : 0u, e->d_child ? 1u : 0u);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->wd_died_init = !e->actors_dirty;
  return AGX_OK;
}

// apply the recorded agx_start_watch calls (the actors' flags are on the device: prepare_run)
agx_status flush_watch_starts(agx_engine* e) {
  AGX_TRY(watch_sync_died(e));
  if (e->wd_starts.empty()) return AGX_OK;
  bool any = false;
  for (const auto& ws : e->wd_starts) {
    if (!ws.count) continue;
    any = true;
    uint32_t *d_w = nullptr, *d_slot = nullptr;
    AGX_TRY(dalloc(&d_slot, ws.count));
    if (!ws.watchees.empty()) {
      AGX_TRY(dalloc(&d_w, ws.watchees.size()));
      HIP_TRY(hipMemcpyAsync(d_w, ws.watchees.data(), ws.watchees.size() * 4ull, hipMemcpyHostToDevice, e->stream));
    }
    const int64_t n = (int64_t)e->n_global;
    const uint32_t off = (uint32_t)(((ws.offset % n) + n) % n);
    const dim3 g((uint32_t)((ws.count + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_watch_start, g, dim3(kThreads), 0, e->stream, e->d_watch, e->d_alive, e->nb, e->bb,
                       (uint32_t)e->n_global, (uint32_t)ws.first, (uint32_t)ws.count, d_w, off, ws.with, ws.payload, d_slot);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_watch_start_due, g, dim3(kThreads), 0, e->stream, e->d_watch, e->nb, e->bb, (uint32_t)e->n_global,
                       (uint32_t)ws.first, (uint32_t)ws.count, d_slot, next_backlog_counts(e));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_watch_start_any, dim3((e->nb + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream, e->d_watch,
                       e->nb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (d_w) hipFree(d_w);
    hipFree(d_slot);
  }
  e->wd_starts.clear();
  if (!any) return AGX_OK;
  e->inflight_known = false;
  // a conflicting actor was stopped on the device: the host's flags follow (they may be the newer ones otherwise)
  std::vector<uint8_t> al(e->n_local);
  AGX_TRY(copy_sync(e, al.data(), e->d_alive, e->n_local, hipMemcpyDeviceToHost));
  for (uint64_t l = 0; l < e->n_local; ++l)
    if (!(al[l] & 1u)) e->h_alive[l] &= 0xFEu;
  uint32_t full = 0;
  AGX_TRY(copy_sync(e, &full, e->d_watch + kWdFull, 4, hipMemcpyDeviceToHost));
  if (full)
    return set_err(AGX_ECAPACITY, "a watch found every one of its actor's %u watch slots taken: the watch is not recorded "
                   "(agx_set_death_watch; at most %u watched refs per actor)", e->wd_slots, AGX_MAX_WATCH_SLOTS);
  return AGX_OK;
}

// the bookkeeping words of the watch storage: [0, kWdBucketOff) then due / mark / clock / watching per bucket
agx_status read_watch_head(agx_engine* e, std::vector<uint32_t>& h) {
  h.assign(kWdBucketOff + 4ull * e->nb, 0u);
  return copy_sync(e, h.data(), e->d_watch, h.size() * 4ull, hipMemcpyDeviceToHost);
}

// after a run: the ticks that passed while the engine was active (the device's last active tick against the
// clock before the run), and the clock now
agx_status watch_after_run(agx_engine* e) {
  if (!e->d_watch) return AGX_OK;
  uint32_t la = 0, clk = 0;
  AGX_TRY(copy_sync(e, &la, e->d_watch + kWdLastAct, 4, hipMemcpyDeviceToHost));
  AGX_TRY(copy_sync(e, &clk, e->d_watch + kWdBucketOff + 2ull * e->nb, 4, hipMemcpyDeviceToHost));
  if (la > e->wd_clock) e->wd_ticks += la - e->wd_clock;
  e->wd_clock = clk;
  return AGX_OK;
}

// ---- supervision (agx_set_supervision)
agx_status read_counters(agx_engine* e, uint64_t* s);
size_t super_words(const agx_engine* e) {
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  return sv_ent_off(e->nb) + kSvEntWords + 2ull * e->sv_levels * npad + (npad + 3ull) / 4ull;
}

// The supervision storage (agx_device.h SuperDev) -- sized by n_local: everything zero (no restart counted, no
// deadline), then the levels and the entries
agx_status alloc_super(agx_engine* e) {
  // (the backoff rows belong to the entries they were checked against: another table drops them)
  if (e->d_backoff && (e->bo_levels != e->sv_levels || e->bo_beh != e->sv_beh ||
                       memcmp(e->bo_sv.data(), e->sv_tab.data(), e->sv_tab.size() * sizeof(agx_supervisor)) != 0)) {
    hipFree(e->d_backoff);
    e->d_backoff = nullptr;
    e->bo_tab.clear();
    if (e->d_super) HIP_TRY(hipMemsetAsync(e->d_super + kSvBackoff, 0, 8, e->stream));
    drop_graphs(e);  // (the launched instantiation is the supervision one again)
  }
  if (!e->d_super) {
    const size_t total = super_words(e);
    if (hipMalloc((void**)&e->d_super, total * 4ull) != hipSuccess) {
      (void)hipGetLastError();
      e->d_super = nullptr;
      return set_err(AGX_ENOMEM, "the supervision state of %llu actors (%u levels, %llu MB) does not fit on the device",
                     (unsigned long long)((uint64_t)e->nb << e->bb), e->sv_levels, (unsigned long long)(total >> 18));
    }
    HIP_TRY(hipMemsetAsync(e->d_super, 0, total * 4ull, e->stream));
    e->sv_init_dirty = true;
    drop_graphs(e);  // (a kernel argument of the captured supersteps)
  }
  const uint32_t head[2] = {e->sv_levels, e->sv_beh};
  HIP_TRY(hipMemcpyAsync(e->d_super, head, sizeof(head), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_super + sv_ent_off(e->nb), e->sv_tab.data(), e->sv_tab.size() * sizeof(agx_supervisor),
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return AGX_OK;
}

// the kinds the actors were registered with (before a run: registrations since the last upload)
agx_status upload_super_init(agx_engine* e) {
  if (!e->sv_init_dirty) return AGX_OK;
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  uint32_t* const at = e->d_super + sv_ent_off(e->nb) + kSvEntWords + 2ull * e->sv_levels * npad;
  AGX_TRY(copy_sync(e, at, e->h_init.data(), e->n_local, hipMemcpyHostToDevice));
  e->sv_init_dirty = false;
  return AGX_OK;
}

// after a run: the ticks so far are the supersteps with mail; the launches of a replay after quiescence advanced
// the clocks and not the time, so the clock's base follows (tick = clock + 1 - base)
agx_status super_after_run(agx_engine* e) {
  if (!e->d_super) return AGX_OK;
  uint64_t s[kStatBlk];
  AGX_TRY(read_counters(e, s));
  e->sv_ticks = s[ST_STEPS] + e->host_steps;
  AGX_TRY(copy_sync(e, &e->sv_clock, e->d_super + kSvBucketOff, 4, hipMemcpyDeviceToHost));
  const uint32_t base = e->sv_clock - (uint32_t)e->sv_ticks;
  return copy_sync(e, e->d_super + kSvBase, &base, 4, hipMemcpyHostToDevice);
}

// ---- children (agx_set_children)
// the death ticks of the child blocks start as "none" (written once, at agx_set_children)
static __global__ void __launch_bounds__(kThreads) k_child_init(uint32_t* wd, uint32_t nb, uint32_t bb, uint32_t first,
                                                               uint32_t count) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  uint32_t* const died = wd + wd_slot_off(nb) + 4ull * wd[0] * (nb << bb);
  died[first + i] = kWdNone;
}
// agx_spawn_children on the device: one thread per actor of the range spawns by the rules of a device spawn;
// `child[i]` is the new child's id, or none (the host stages the Create envelopes)
static __global__ void __launch_bounds__(kThreads) k_child_spawn(uint32_t* wd, const uint8_t* alive, uint32_t nb, uint32_t bb,
                                                                uint32_t n, uint32_t first, uint32_t count, uint32_t* child) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const WatchDev WD = watch_dev(wd, nb, bb, n);
  const ChildDev CD = child_dev(wd, nb);
  const uint32_t l = first + i;
  child[i] = kWdNone;
  if (!(alive[l] & 1u) || WD.died[l] != kWdNone) return;  // (a stopped actor spawns nothing)
  child[i] = CD.spawn(l);
}

size_t child_words(const agx_engine* e) { return cd_count_off(e->nb) + ((size_t)e->nb << e->bb); }

// apply the recorded agx_spawn_children calls (the actors' flags and death ticks are on the device: after
// flush_watch_starts); the Create envelopes join the host-staged tells
agx_status flush_child_spawns(agx_engine* e) {
  if (e->ch_spawns.empty()) return AGX_OK;
  for (const auto& cs : e->ch_spawns) {
    if (!cs.count) continue;
    uint32_t* d_ch = nullptr;
    AGX_TRY(dalloc(&d_ch, cs.count));
    hipLaunchKernelGGL(k_child_spawn, dim3((uint32_t)((cs.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, e->stream,
                       e->d_watch, e->d_alive, e->nb, e->bb, (uint32_t)e->n_global, (uint32_t)cs.first, (uint32_t)cs.count, d_ch);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> ch(cs.count);
    const agx_status st = copy_sync(e, ch.data(), d_ch, cs.count * 4ull, hipMemcpyDeviceToHost);
    hipFree(d_ch);
    AGX_TRY(st);
    for (uint64_t i = 0; i < cs.count; ++i) {
      if (ch[i] == kWdNone) continue;
      e->staged_total++;
      e->hs_key.push_back(ch[i]);
      e->hs_src.push_back((uint32_t)(cs.first + i));
      e->hs_pay.push_back((AGX_TAG_CREATE << 24) | (cs.site << AGX_SPAWN_ARG_BITS) | (cs.arg & AGX_SPAWN_ARG_MASK));
    }
  }
  e->ch_spawns.clear();
  e->inflight_known = false;
  return AGX_OK;
}

// ---- the receptionist (agx_set_receptionist)
// apply the recorded agx_register_services calls: the actors' flags reach the device first when the host's are the
// newer ones; each call is the start kernel over the buckets of its range, then the rebuild (the listing is in
// force for the next tick)
agx_status flush_recep_starts(agx_engine* e) {
  if (e->rc_starts.empty() && e->tp_pubs.empty() && e->ls_starts.empty()) return AGX_OK;
  if (e->d_list) hipLaunchKernelGGL(k_listing_mark, dim3(1), dim3(AGX_MAX_SERVICE_KEYS), 0, e->stream, e->d_recep);
  if (e->actors_dirty && !(e->rc_starts.empty() && e->ls_starts.empty())) HIP_TRY(hipMemcpyAsync(e->d_alive, e->h_alive.data(), e->n_local, hipMemcpyHostToDevice, e->stream));
  for (const auto& rs : e->rc_starts) {
    if (!rs.count) continue;
    const uint32_t b0 = (uint32_t)(rs.first >> e->bb), b1 = (uint32_t)((rs.first + rs.count - 1) >> e->bb);
    hipLaunchKernelGGL(k_recep_start, dim3(b1 - b0 + 1), dim3(kRcThreads), 0, e->stream, e->d_recep, e->d_alive, e->bb,
                       (uint32_t)e->n_local, (uint32_t)rs.first, (uint32_t)rs.count, rs.key, rs.on, b0);
    launch_recep_rebuild(e);
    HIP_TRY(hipGetLastError());
  }
  if (e->d_topic) {  // the host's publications join the pending log; then the log is planned against the new counts
    for (const auto& tp : e->tp_pubs)
      hipLaunchKernelGGL(k_topic_host_pub, dim3(1), dim3(1), 0, e->stream, e->d_recep, tp.key, tp.sender, tp.payload,
                         reinterpret_cast<unsigned long long*>(e->d_stats + ST_ERROR));
    launch_topic_plan(e, next_backlog_counts(e), 1u);
    HIP_TRY(hipGetLastError());
    e->inflight_known = false;
  }
  if (e->d_list) {  // the host's subscriptions; then the Listings are planned against the new counts and versions
    for (const auto& ls : e->ls_starts) {
      if (!ls.count) continue;
      const uint32_t b0 = (uint32_t)(ls.first >> e->bb), b1 = (uint32_t)((ls.first + ls.count - 1) >> e->bb);
      hipLaunchKernelGGL(k_listing_start, dim3(b1 - b0 + 1), dim3(kRcThreads), 0, e->stream, e->d_recep, e->d_alive, e->bb,
                         (uint32_t)e->n_local, (uint32_t)ls.first, (uint32_t)ls.count, ls.key, ls.on, b0);
    }
    launch_listing_plan(e, next_backlog_counts(e), 1u);
    HIP_TRY(hipGetLastError());
    e->inflight_known = false;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->rc_starts.clear();
  e->tp_pubs.clear();
  e->ls_starts.clear();
  return AGX_OK;
}

// upload host mirrors / staged tells before a run
agx_status prepare_run(agx_engine* e) {
  if (e->rc_bad_start)
    return set_err(AGX_EINVAL, "agx_register_services was called on an engine without the receptionist (agx_set_receptionist)");
  if (e->beh_recep && !e->d_recep)  // (only the receptionist variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours register, deregister, route, forward or read a listing, but the engine "
                   "has no receptionist (agx_set_receptionist)");
  if (e->d_recep && e->beh_rc_keys > e->rc_keys)
    return set_err(AGX_EINVAL, "the compiled behaviours use service key %u, but the receptionist has %u keys "
                   "(agx_set_receptionist)", e->beh_rc_keys - 1u, e->rc_keys);
  if (e->beh_route_two >= 0)
    return set_err(AGX_EINVAL, "compiled behaviours: route action %lld sets more than one of AGX_ROUTE_BY_INDEX, "
                   "AGX_ROUTE_HASHED and AGX_ROUTE_RANDOM", (long long)e->beh_route_two);
  if (e->beh_router && !e->d_hash)  // (only the router-logics variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours route by consistent hashing or at random, but the engine has no "
                   "router logics (agx_set_router_logics)");
  if (e->beh_hashed_keys & ~e->hr_mask)
    return set_err(AGX_EINVAL, "the compiled behaviours route by consistent hashing through service key %u, which is not a "
                   "hashed key (agx_set_router_logics: hashed_keys_mask 0x%x)",
                   (uint32_t)__builtin_ctz(e->beh_hashed_keys & ~e->hr_mask), e->hr_mask);
  if (e->beh_publish && !e->d_topic)  // (only the topic variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours publish, but the engine has no topics (agx_set_topics)");
  if (e->beh_listing && !e->d_list)  // (only the listings variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours subscribe to or find a listing, but the engine has no listings "
                   "(agx_set_listings)");
  if (e->ch_bad_spawn)
    return set_err(AGX_EINVAL, "agx_spawn_children was called on an engine without children (agx_set_children)");
  if (e->beh_child && !e->d_child)  // (only the children variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours spawn, stop a child or read the spawn count, but the engine has no "
                   "children (agx_set_children)");
  if (e->d_child) {
    if (e->beh_ctl_tags)
      return set_err(AGX_EINVAL, "the compiled behaviours name message tag 0xFD or 0xFC, reserved for Create and Stop "
                     "envelopes on an engine with children");
    for (const auto& st : e->ch_sites)
      if (st.kind - AGX_KIND_COMPILED >= e->n_beh)
        return set_err(AGX_EINVAL, "children: a spawn site's kind %u is no compiled behaviour of the tables (%u behaviours)",
                       st.kind, e->n_beh);
    if (!e->started)
      for (const auto& r : e->ch_regions)
        for (uint64_t x = r.first_child; x < (uint64_t)r.first_child + (uint64_t)r.n_parents * r.max_children; ++x)
          if (e->h_alive[x] & 1u)
            return set_err(AGX_EINVAL, "children: id %llu of a child block is registered", (unsigned long long)x);
  }
  if ((e->beh_fail || e->beh_svsig) && !e->sv_on)  // (only the supervision variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours fail (AGX_RES_FAIL) or hold a PreRestart / PostStop signal case, but "
                   "the engine has no supervision (agx_set_supervision)");
  if (e->sv_on && (e->beh_watch || e->beh_tm_keys || e->beh_stash || e->beh_vstash))
    return set_err(AGX_EINVAL, "the compiled behaviours of an engine with supervision (agx_set_supervision) %s",
                   e->beh_watch ? "watch, unwatch or hold a Terminated signal case: death watch needs an engine of its own"
                   : e->beh_tm_keys ? "use timers: timers need an engine of their own"
                                    : "stash, unstash_all or read the stash size: a stash needs an engine of its own");
  if (e->sv_on && e->beh_sv_tells > e->kmax)
    return set_err(AGX_EINVAL, "supervision: within one behaviour a case that fails or stops and the largest PreRestart / "
                   "PostStop case tell %u times together, max_emit is %u", e->beh_sv_tells, e->kmax);
  if (e->wd_bad_start)
    return set_err(AGX_EINVAL, "agx_start_watch was called on an engine without death watch (agx_set_death_watch)");
  if (e->beh_watch && !e->wd_slots)  // (only the watch variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours watch, unwatch or hold a signal case, but the engine has no death "
                   "watch (agx_set_death_watch)");
  if (e->rt_bad_start)
    return set_err(AGX_EINVAL, "agx_start_receive_timeout was called on an engine without receive timeouts "
                   "(agx_set_receive_timeout)");
  if (e->beh_rt && !e->rt_on)  // (only the receive-timeout variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours set or cancel a receive timeout, but the engine has no receive "
                   "timeouts (agx_set_receive_timeout)");
  if (e->rt_on && e->beh_rt_tag)
    return set_err(AGX_EINVAL, "the compiled behaviours name message tag 0xFB, reserved for receive-timeout envelopes on an "
                   "engine with receive timeouts");
  if (e->beh_passivate && !e->d_shard)  // (only the sharding variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours passivate, but the engine has no sharding (agx_set_sharding)");
  for (const auto& t : e->sh_types)
    if (t.kind - AGX_KIND_COMPILED >= e->n_beh)
      return set_err(AGX_EINVAL, "sharding: an entity type's kind %u is no compiled behaviour of the tables (%u behaviours)",
                     t.kind, e->n_beh);
  if (e->beh_ask_keys && !e->ask_on)  // (only the ask variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours ask, but the engine has no ask pattern (agx_set_ask)");
  if (e->beh_ask_unpaired >= 0)
    return set_err(AGX_EINVAL, "the compiled behaviours' action %lld is half an ask: AGX_A_ASK_SEND comes directly after the "
                   "AGX_A_ASK_ARM of the same key", (long long)e->beh_ask_unpaired);
  if (e->beh_ask_keys > e->tm_keys)
    return set_err(AGX_EINVAL, "the compiled behaviours ask on timer key %u, but the engine has %u slots per actor "
                   "(agx_set_timers)", e->beh_ask_keys - 1u, e->tm_keys);
  if (e->tm_bad_start)
    return set_err(AGX_EINVAL, "agx_start_timers was called on an engine without timers (agx_set_timers)");
  if (e->beh_tm_keys > e->tm_keys)  // (only the timer variant interprets those: loud, never wrong)
    return set_err(AGX_EINVAL, e->tm_keys ? "the compiled behaviours use timer key %u, but the engine has %u timer slots per "
                   "actor (agx_set_timers)" : "the compiled behaviours use timers (key %u), but the engine has none "
                   "(agx_set_timers; it has %u slots)", e->beh_tm_keys - 1u, e->tm_keys);
  if (e->beh_stash && !e->stash_on)  // (only the stash variant interprets those results: loud, never wrong)
    return set_err(AGX_EINVAL, "the compiled behaviours stash or unstash_all, but no mailbox class of this engine has a "
                   "stash capacity (agx_set_stash): without one every stash would overflow");
  if (e->actors_dirty) {
    HIP_TRY(hipMemcpyAsync(e->d_kind, e->h_kind.data(), e->n_local, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_alive, e->h_alive.data(), e->n_local, hipMemcpyHostToDevice, e->stream));
    // first upload of a CRDT engine: actor-major rows from now on -- except delta-CRDT counter
    // populations, which stay word-major: there a lane walks its own replica's envelope and log,
    // and consecutive lanes then read consecutive words (same-box A/B: GCounter delta 3.25e9 ->
    // 3.93e9 word-major; ORSet delta 1.29e9 actor-major vs 1.17e9 word-major, its element rows
    // are read whole).  AGX_CRDT_LAYOUT=actor|word overrides.
    const char* lay = getenv("AGX_CRDT_LAYOUT");
    const bool word_major = apply_variant(e) != V_OR && apply_variant(e) != V_LWWMAP &&  // (k_orset_merge / k_lwwmap_merge walk actor-major rows)
                            apply_variant(e) != V_PNCMAP &&                              // (k_pncmap_merge too)
                            apply_variant(e) != V_ORMM &&                                // (and k_ormm_merge)
                            apply_variant(e) != V_LWWMAP_DELTA &&                        // (and k_lwwmap_delta_merge)
                            (lay ? lay[0] == 'w' : (e->delta_max && !(e->kinds_mask & kb(AGX_KIND_ORSET))));
    if (e->pw && !e->pitch && !word_major) {
      const uint32_t pitch = e->W <= 16 ? (e->W + 1u) & ~1u : (e->W + 15u) & ~15u;
      uint64_t* d = nullptr;
      AGX_TRY(dalloc(&d, (uint64_t)e->n_local * pitch));
      HIP_TRY(hipFree(e->d_state));
      e->d_state = d;
      e->pitch = pitch;
      drop_graphs(e);  // (the state array is a kernel argument)
    }
    if (e->pitch) {  // word-major mirror -> actor-major rows
      std::vector<uint64_t> rows((size_t)e->n_local * e->pitch, 0);
      for (uint64_t w = 0; w < e->W; ++w)
        for (uint64_t l = 0; l < e->n_local; ++l) rows[l * e->pitch + w] = e->h_state[w * e->n_local + l];
      HIP_TRY(hipMemcpyAsync(e->d_state, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(e->d_state, e->h_state.data(), e->n_local * e->W * 8, hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->actors_dirty = false;
    e->wd_died_init = false;  // (actors registered since: their death ticks follow below)
    e->sv_init_dirty = e->sv_on;  // (... their initial kinds)
    e->prio_dirty = e->prio_mask != 0;  // (mailboxes bound since: the per-bucket marks below)
    e->stash_dirty = e->stash_on;
  }
  if (e->stash_dirty) AGX_TRY(upload_stash(e));
  if (e->tm_keys) {
    AGX_TRY(alloc_timers(e));
    AGX_TRY(flush_timer_starts(e));
  }
  if (e->wd_slots) {
    AGX_TRY(alloc_watch(e));
    AGX_TRY(flush_watch_starts(e));
    if (e->d_child) AGX_TRY(flush_child_spawns(e));
  }
  if (e->sv_on) {
    AGX_TRY(alloc_super(e));
    AGX_TRY(upload_super_init(e));
  }
  if (e->d_recep) AGX_TRY(flush_recep_starts(e));
  if (e->prio_dirty) {  // priority tables and the buckets that hold an actor of a prioritised class
    std::vector<uint8_t> pb(e->prio_tab);  // tables, then the bucket marks (kPrioBucketOff)
    pb.resize(kPrioBucketOff + e->nb, 0);
    for (uint64_t l = 0; l < e->n_local; ++l)
      if ((e->prio_mask >> ((e->h_alive[l] >> 1) & (AGX_MAX_MAILBOX_CLASSES - 1))) & 1u) pb[kPrioBucketOff + (l >> e->bb)] = 1;
    if (!e->d_ptab) {
      AGX_TRY(dalloc(&e->d_ptab, pb.size()));
      drop_graphs(e);  // (a kernel argument of the captured supersteps)
    }
    HIP_TRY(hipMemcpyAsync(e->d_ptab, pb.data(), pb.size(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->prio_dirty = false;
  }
  if (e->fused && !e->hs_key.empty()) {
    // staged tells still on the device (a run of 0 supersteps) come first: staging order
    if (e->stg_pending) {
      e->hs_key.insert(e->hs_key.begin(), e->hd_key.begin(), e->hd_key.end());
      e->hs_src.insert(e->hs_src.begin(), e->hd_src.begin(), e->hd_src.end());
      e->hs_pay.insert(e->hs_pay.begin(), e->hd_pay.begin(), e->hd_pay.end());
    }
    const uint64_t n = e->hs_key.size();
    if (n > e->stg_cap) {
      free_msgs(e->stg);
      AGX_TRY(alloc_msgs(e->stg, n));
      e->stg_cap = n;
      drop_graphs(e);  // the staging arena is a kernel argument of the captured supersteps
    }
    // stable counting sort by destination bucket: each bucket's staged tells are one run
    std::vector<uint32_t> off(e->nb + 1, 0), cnt(e->nb, 0);
    for (uint64_t i = 0; i < n; ++i) cnt[e->hs_key[i] >> e->bb]++;
    for (uint32_t b = 0; b < e->nb; ++b) off[b + 1] = off[b] + cnt[b];
    std::vector<uint32_t> k(n), sv(n), pv(n), pos(off.begin(), off.end() - 1);
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t o = pos[e->hs_key[i] >> e->bb]++;
      k[o] = e->hs_key[i];
      sv[o] = e->hs_src[i];
      pv[o] = e->hs_pay[i];
    }
    HIP_TRY(hipMemcpyAsync(e->stg.key, k.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->stg.src, sv.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->stg.pay, pv.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_stg_off, off.data(), e->nb * 4ull, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_stg_cnt, cnt.data(), e->nb * 4ull, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->hd_key.swap(e->hs_key);
    e->hd_src.swap(e->hs_src);
    e->hd_pay.swap(e->hs_pay);
    e->hs_key.clear();
    e->hs_src.clear();
    e->hs_pay.clear();
    e->stg_pending = true;
  }
  if (!e->hs_key.empty()) {
    uint64_t n = e->hs_key.size();
    if (n > e->stg_cap) {
      free_msgs(e->stg);
      AGX_TRY(alloc_msgs(e->stg, n));
      e->stg_cap = n;
    }
    HIP_TRY(hipMemcpyAsync(e->stg.key, e->hs_key.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->stg.src, e->hs_src.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->stg.pay, e->hs_pay.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->n_staged_dev = (uint32_t)n;
    e->hs_key.clear();
    e->hs_src.clear();
    e->hs_pay.clear();
  }
  return AGX_OK;
}

// ----------------------------------------------------------- multi-rank step
// phase 1: backlog chunks -> front of A; the apply's owner-grouped tells -> s2, owner-major
// (the stable owner partition of the tells in chunk order); count vector
// [send counts..., n_backlog, n_staged] for the all-gather.
// direct: the device-resident replay of plain behaviours -- the peers' runs go straight into their send
// slabs (k_mcompact_copy), k_mr_pack copies only the own run
agx_status phase1(agx_engine* e, bool direct = false) {
  McompactArgs m{};
  m.ch = make_chunks(e);
  m.eg = e->eg0.c();
  m.tcnt = e->d_tcnt[0];
  m.toff = e->d_toff[0];
  m.out0 = e->A.m();
  m.out1 = e->s2.m();
  m.off0 = e->d_moff0;
  m.off1 = e->d_moff1;
  m.d_total = e->d_total;
  m.cvec = e->d_cvec;
  m.alive = e->d_alive;
  m.stopq = e->d_stopq;
  m.nstop = e->d_nstop;
  m.stats = e->d_stats;
  m.step = e->pw ? e->d_step : nullptr;
  m.heap_top = e->d_heap_top;
  m.skew_n = e->d_skew_n;
  m.cap0 = e->cap;
  m.cap1 = e->cap_emit;
  m.R = e->R;
  m.tstride = e->tstride;
  m.n_staged = e->n_staged_dev;
  m.halt = e->d_halt;  // (multi-rank only; zero outside device-resident replays)
  m.dense_left = e->d_dense_left;
  m.sslab = direct ? e->d_sslab : nullptr;
  m.slab = e->slab;
  m.rank = e->rank;
  {
    Scope s(e, K_MCOMPACT);
    hipLaunchKernelGGL(k_mcompact_scan, dim3(1), dim3(kScanThreads), 0, e->stream, m);
    hipLaunchKernelGGL(k_mcompact_copy, dim3(grid_for(e->nb, 4096)), dim3(kThreads), 0, e->stream, m);
  }
  if (e->pw) {
    Scope s(e, K_MCOMPACT);
    hipLaunchKernelGGL(k_pack_rows, dim3(grid_for(e->cap_emit / kThreads + 1, 2048)), dim3(kThreads), 0, e->stream,
                       e->s2.c(), e->d_total, make_params(e), e->d_s2rows);
  }
  HIP_TRY(hipGetLastError());
  return AGX_OK;
}

// phase 2: staged tells after the received mail, group by bucket, apply.
agx_status phase2(agx_engine* e, uint64_t n_sorted, uint64_t staged_at) {
  if (e->n_staged_dev) {
    HIP_TRY(hipMemcpyAsync(e->A.key + staged_at, e->stg.key, e->n_staged_dev * 4ull, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->A.src + staged_at, e->stg.src, e->n_staged_dev * 4ull, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->A.pay + staged_at, e->stg.pay, e->n_staged_dev * 4ull, hipMemcpyDeviceToDevice, e->stream));
    e->n_staged_dev = 0;
  }
  hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(64), 0, e->stream, e->d_n, (uint32_t)n_sorted);  // no DMA round trip
  DevMsgs* sorted = nullptr;
  AGX_TRY(launch_bucket_sort(e, false, &sorted));
  AGX_TRY(launch_apply(e, *sorted));
  return AGX_OK;
}

struct Plan {
  uint64_t total_inflight = 0;
  uint64_t n_bl = 0, n_recv = 0, n_staged = 0;
  std::vector<uint64_t> send_cnt, send_off, recv_cnt, recv_off;
};

void make_plan(agx_engine* e, const uint64_t* mat, Plan& p) {
  const uint32_t R = e->R, S = R + 2;
  p.send_cnt.assign(R, 0);
  p.send_off.assign(R, 0);
  p.recv_cnt.assign(R, 0);
  p.recv_off.assign(R, 0);
  p.total_inflight = 0;
  for (uint32_t r = 0; r < R; ++r)
    for (uint32_t c = 0; c < S; ++c) p.total_inflight += mat[r * S + c];
  p.n_bl = mat[e->rank * S + R];
  p.n_staged = mat[e->rank * S + R + 1];
  uint64_t so = 0, ro = p.n_bl;
  for (uint32_t q = 0; q < R; ++q) {
    p.send_cnt[q] = mat[e->rank * S + q];
    p.send_off[q] = so;
    so += p.send_cnt[q];
    p.recv_cnt[q] = mat[q * S + e->rank];
    p.recv_off[q] = ro;
    ro += p.recv_cnt[q];
  }
  p.n_recv = ro - p.n_bl;
}

// host <-> device copies of the agx_set_* / read-back entry points: on the engine stream, waited for
// (ordered after any work still queued there -- never a null-stream copy racing the non-blocking
// engine stream)
agx_status copy_sync(agx_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return AGX_OK;
}

// the reply path: move the device outbox to the host queue (the engine is idle between calls); the
// appends past the outbox capacity were dropped on the device and are counted into outbox_lost
agx_status drain_outbox(agx_engine* e) {
  if (!e->d_outbox_n) return AGX_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  uint32_t cnt = 0;
  AGX_TRY(copy_sync(e, &cnt, e->d_outbox_n, 4, hipMemcpyDeviceToHost));
  const uint64_t m = e->d_outbox ? std::min<uint64_t>(cnt, e->outbox_cap) : 0;
  if (m) {
    const size_t o = e->outq.size();
    e->outq.resize(o + 3 * m);
    AGX_TRY(copy_sync(e, e->outq.data() + o, e->d_outbox, 12 * m, hipMemcpyDeviceToHost));
  }
  e->outbox_lost += cnt - m;
  const uint32_t zero = 0;
  if (cnt) AGX_TRY(copy_sync(e, e->d_outbox_n, &zero, 4, hipMemcpyHostToDevice));
  return AGX_OK;
}

// bring the host mirrors up to date with the device (commits pending stops)
agx_status sync_mirrors(agx_engine* e) {
  if (e->actors_dirty) return AGX_OK;  // host mirror is newer than the device
  hipLaunchKernelGGL(k_commit_stops, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_alive, e->d_stopq, e->d_nstop);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  AGX_TRY(copy_sync(e, e->h_alive.data(), e->d_alive, e->n_local, hipMemcpyDeviceToHost));
  // (the kinds too: become, unstash_all, a restart, a child's Create and an entity's start change them on the
  // device, and the next upload writes the whole mirror back; h_init keeps the registered kinds)
  AGX_TRY(copy_sync(e, e->h_kind.data(), e->d_kind, e->n_local, hipMemcpyDeviceToHost));
  if (e->pitch) {  // actor-major rows -> word-major mirror
    std::vector<uint64_t> rows((size_t)e->n_local * e->pitch);
    AGX_TRY(copy_sync(e, rows.data(), e->d_state, rows.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t w = 0; w < e->W; ++w)
      for (uint64_t l = 0; l < e->n_local; ++l) e->h_state[w * e->n_local + l] = rows[l * e->pitch + w];
  } else {
    AGX_TRY(copy_sync(e, e->h_state.data(), e->d_state, e->n_local * e->W * 8, hipMemcpyDeviceToHost));
  }
  return AGX_OK;
}

// One read-back of every counter: the apply's per-block counters are summed and the messages in
// flight (backlog + tells of the last apply + staged) counted on the device, into the d_stats
// block, which comes back with ONE copy and ONE stream sync.
agx_status read_counters(agx_engine* e, uint64_t* s) {
  hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_bstats, kMaxApplyGrid, e->d_sred);
  if (e->fused)
    hipLaunchKernelGGL(k_inflight_fused, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_blc[0], e->d_blc[1],
                       e->d_emc[0], e->d_emc[1], e->d_stg_cnt, e->par ^ 1u, e->nb, (unsigned long long*)e->d_inflight);
  else
    hipLaunchKernelGGL(k_inflight, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_chunk_cnt, e->nchunks,
                       (unsigned long long*)e->d_inflight, e->ring_live || e->rg_on ? e->d_ring_total : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(e->h_stat, e->d_stats, kStatBlk * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  memcpy(s, e->h_stat, kStatBlk * 8);
  return AGX_OK;
}

// The kernels' sticky error word -> status.  The bits are never cleared: after a capacity
// overflow mail was dropped, after a counter wrap a slot is wrong, so every later result of the
// engine is suspect -- each later agx_run / agx_get_stats reports the same error (agx_get_stats
// still fills its counters); destroy the engine and start over.
agx_status error_status(const agx_engine* e, uint64_t err) {
  if (err & kErrRange)
    return set_err(AGX_ERANGE, "a GCounter/PNCounter/PNCounterMap slot exceeded 2^64 - 1 (u64 slots; the reference uses BigInt) or an "
                   "ORSet / LWWMap / PNCounterMap / ORMultiMap replica's own version (an ORMultiMap value set's included) exceeded 2^32 - 1 "
                   "(u32 versions; the reference uses Long) or an LWWMap "
                   "timestamp would pass the int64 range (the reference's Long would wrap)");
  if (err & kErrPrioTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors that holds a priority-mailbox actor received more than one "
                   "tile of %d messages (backlog included): a prioritised actor's queue is ordered within one tile "
                   "(smaller agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrStashTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors that holds an actor of a deque-based mailbox class received "
                   "more than one tile of %d messages (backlog and released stash messages included): a stash is "
                   "drained within one tile (smaller agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrTimerTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors of an engine with timers received more than one tile of %d "
                   "messages (backlog and the tick's timer messages included): the launches for larger inboxes know "
                   "no timers (smaller agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrWatchTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors of an engine with death watch received more than one tile of %d "
                   "messages (backlog and the tick's Terminated envelopes included): the launches for larger inboxes "
                   "know no death watch (smaller agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrSuperTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors of an engine with supervision received more than one tile of %d "
                   "messages (backlog included): the launches for larger inboxes know no supervision (smaller "
                   "agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrRecepTile)
    return set_err(AGX_ECAPACITY, "a bucket of %u actors of an engine with the receptionist received more than one tile of "
                   "%d messages (backlog included): the launches for larger inboxes know no receptionist (smaller "
                   "agx_cfg.bucket_actors spread the load)", 1u << e->bb, kBucket);
  if (err & kErrRecepCap)
    return set_err(AGX_ECAPACITY, "a service key's listing would hold more than %u ids, the receptionist's capacity "
                   "(agx_set_receptionist): the listing keeps its first %u ids", e->rc_cap, e->rc_cap);
  if (err & kErrTopicLog)
    return set_err(AGX_ECAPACITY, "a tick's publications would exceed the topics' log capacity of %u entries (agx_set_topics): "
                   "the publications past it are lost", e->tp_cap);
  if (err & kErrWatchSlots)
    return set_err(AGX_ECAPACITY, "a watch found every one of its actor's %u watch slots taken: the watch is not recorded "
                   "(agx_set_death_watch; at most %u watched refs per actor)", e->wd_slots, AGX_MAX_WATCH_SLOTS);
  if (err & kErrCapacity)
    return set_err(AGX_ECAPACITY, "in-flight messages exceeded engine capacity (msg_capacity=%llu)",
                   (unsigned long long)e->cap);
  if (err & kErrBarrier)
    return set_err(AGX_EDEVICE, "a persistent superstep launch's grid barrier timed out (not every block was "
                   "resident); unset AGX_PERSIST to avoid the persistent launch");
  return AGX_OK;
}

// counters -> agx_stats (filled even when an error is reported); check: report an error
// recorded by the kernels
agx_status collect_stats(agx_engine* e, agx_stats* out, bool check) {
  uint64_t s[kStatBlk];
  AGX_TRY(read_counters(e, s));
  e->inflight_dev = s[kStatInfl];  // (exact until the next agx_run: agx_stage_tells' capacity check)
  e->inflight_known = true;
  const agx_status est = check ? error_status(e, s[ST_ERROR]) : AGX_OK;
  const uint64_t* bs = s + kStatSred;
  agx_stats st{};
  st.delivered = bs[0];
  st.dead_letters = s[ST_DEAD] + bs[1] + e->staged_dead;
  st.unhandled = bs[2];
  st.emitted = bs[3];
  st.staged = e->staged_total;
  st.supersteps = s[ST_STEPS] + e->host_steps;
  // backlog + tells produced by the last apply, plus host tells not yet consumed
  st.in_flight = s[kStatInfl] + e->n_staged_dev + e->hs_key.size();
  if (e->stash_on) {  // every buffered and parked message is in flight; the next windows are in the backlog counts
    uint64_t held, pending, windows;
    AGX_TRY(stash_scan(e, &held, &pending, &windows));
    st.in_flight += held + pending - windows;
  }
  if (e->d_timers) {  // the backlog counts carry the next tick's fires: not sent yet, not in flight
    std::vector<uint32_t> h;
    AGX_TRY(read_timer_head(e, h));
    for (uint32_t b = 0; b < e->nb; ++b) st.in_flight -= std::min<uint64_t>(st.in_flight, h[kTmBucketOff + e->nb + b]);
  }
  if (e->d_watch) {  // the backlog counts carry the due slots: their envelopes are not sent yet, not in flight
    std::vector<uint32_t> h;
    AGX_TRY(read_watch_head(e, h));
    for (uint32_t b = 0; b < e->nb; ++b) st.in_flight -= std::min<uint64_t>(st.in_flight, h[kWdBucketOff + b]);
  }
  // B = E_in + f_out*E_out + 2*S*(A/M); kind+alive bytes read per activation.
  // S = the state words a behaviour touches: words 0-1 (plain and compiled behaviours), a CRDT's
  // data words (a full-state merge reads and writes all of them), or with delta-CRDT replication
  // the envelope/selector words plus one element (a delta touches a few elements; rows not counted).
  uint64_t sw = std::min<uint64_t>(e->W, 2);
  const uint32_t km = e->kinds_mask;
  if (km & kb(AGX_KIND_GCOUNTER)) sw = std::max<uint64_t>(sw, AGX_GCOUNTER_WORDS);
  if (km & kb(AGX_KIND_PNCOUNTER)) sw = std::max<uint64_t>(sw, AGX_PNCOUNTER_WORDS);
  if (km & kb(AGX_KIND_ORSET)) sw = std::max<uint64_t>(sw, e->delta_max ? AGX_DELTA_ENV_WORDS + 4 : AGX_ORSET_WORDS);
  if (km & kb(AGX_KIND_LWWMAP)) sw = std::max<uint64_t>(sw, AGX_LWWMAP_WORDS);
  if (km & kb(AGX_KIND_PNCOUNTERMAP)) sw = std::max<uint64_t>(sw, AGX_PNCMAP_WORDS);
  if (km & kb(AGX_KIND_ORMULTIMAP)) sw = std::max<uint64_t>(sw, AGX_ORMM_WORDS);
  st.bytes_alg = 12ull * st.delivered + 12ull * st.emitted + (16ull * std::min<uint64_t>(sw, e->W) + 2ull) * bs[4];
  if (out) *out = st;
  return est;
}

// one superstep on one rank: [chunks] -> group by bucket -> in-bucket sort + drain + apply -> [chunks]
agx_status launch_step_single(agx_engine* e) {
  if (e->fused) return launch_apply(e, e->A);  // one kernel per superstep
  AGX_TRY(launch_staged_chunk(e));
  DevMsgs* sorted = nullptr;
  AGX_TRY(launch_bucket_sort(e, true, &sorted));
  AGX_TRY(launch_apply(e, *sorted));
  return AGX_OK;
}

// The persistent fused launch: a strict replay whose every superstep is the dense
// launch alone runs its K supersteps in ONE launch of k_dense_fused<.., true> -- one block per bucket,
// a grid barrier between supersteps, the actors' state words kept in registers -- instead of K
// launches.  Only when all nb blocks are resident at once (the barrier waits for every block): nb <=
// resident blocks per CU x CUs.  Opt-in (AGX_PERSIST=1): 3.8x slower than K graph-replayed launches on
// the 1M ring (47 vs 12.5 us per superstep) -- the grid barrier costs more than a
// kernel boundary.
bool persist_ok(agx_engine* e) {
  const uint32_t vid = apply_variant(e);
  if (e->persist >= 0 && e->persist_vid != vid) e->persist = -1;  // (kinds registered since: re-decide)
  if (e->persist < 0) {
    e->persist_vid = vid;
    e->persist = 0;
    const char* k = getenv("AGX_PERSIST");
    int per_cu = 0, dev = 0, ncu = 0;
    if (k && atoi(k) != 0 && e->R == 1 && e->fused &&
        agx_dense_persist_occupancy(vid, &per_cu) == hipSuccess && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      e->persist = (uint64_t)e->nb <= (uint64_t)per_cu * (uint64_t)ncu ? 1 : 0;
    (void)hipGetLastError();
  }
  return e->persist == 1 && active_feature(e) == F_NONE && e->fused && e->strict_cap && e->dense_alone && dense_on(e, vid) && !e->skew_only &&
         !e->recover_dense;
}

// hipGraph of `steps` supersteps (the launch-bound inner loop): replayed
// instead of 10+ eager launches per superstep.
agx_status capture_steps(agx_engine* e, uint32_t steps, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  agx_status st = AGX_OK;
  e->captured_persist = false;
  if (steps > 1 && persist_ok(e)) {  // one persistent launch for the replay's supersteps
    e->cur_slot = 0;
    e->persist_steps = steps;
    st = launch_step_single(e);
    e->persist_steps = 0;
    e->captured_persist = true;
  } else {
    for (uint32_t i = 0; i < steps && st == AGX_OK; ++i) {
      e->cur_slot = i;  // fused: the i-th superstep of the replay reports its inbox sizes in row i
      st = launch_step_single(e);
    }
  }
  e->cur_slot = 0;
  if (st == AGX_OK && e->fused)  // the replay's rows and abort marks -> host ring slot (no D2H copy)
    hipLaunchKernelGGL(k_replay_out, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_cntb, steps * e->nb,
                       e->strict_cap ? e->d_abort : nullptr, (const unsigned long long*)(e->d_stats + ST_ERROR), e->d_ring,
                       e->d_rctr, agx_engine::kGraphSteps * e->nb + kRingTail);
  hipError_t ce = hipStreamEndCapture(e->stream, &g);
  if (st) {
    if (g) hipGraphDestroy(g);
    return st;
  }
  if (ce != hipSuccess) return set_err(AGX_EDEVICE, "hipStreamEndCapture: %s", hipGetErrorString(ce));
  hipError_t ie = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (ie != hipSuccess) return set_err(AGX_EDEVICE, "hipGraphInstantiate: %s", hipGetErrorString(ie));
  // upload now: a graph's first launch would otherwise pay the upload inside the budget that
  // first replays it (the 8-superstep graphs are first used by longer runs than the warmup)
  hipError_t ue = hipGraphUpload(*out, e->stream);
  if (ue != hipSuccess) return set_err(AGX_EDEVICE, "hipGraphUpload: %s", hipGetErrorString(ue));
  return AGX_OK;
}

agx_status run_single(agx_engine* e, uint32_t max_steps) {
  constexpr uint32_t kLag = 4;  // replays in flight before the host polls quiescence
  for (auto& x : e->lag_ev)
    if (!x) HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
  hipEvent_t* ev = e->lag_ev;
  agx_status st = AGX_OK;
  uint32_t left = max_steps;
  // LWWMap engines: k_lwwmap_merge's logical time is the superstep's number among the supersteps with mail.  Those
  // are the first supersteps of a run, so the supersteps launched below have the numbers lww_next + 1, ..., from the
  // count so far; every launch is preceded, in stream order, by the number its first superstep follows (the empty
  // supersteps a replay runs after quiescence draw no timestamp)
  uint32_t lww_next = 0;
  if (e->d_lww_step0 && left) {
    uint64_t dsteps = 0;
    AGX_TRY(copy_sync(e, &dsteps, e->d_stats + ST_STEPS, 8, hipMemcpyDeviceToHost));
    lww_next = (uint32_t)(dsteps + e->host_steps);
  }
  auto lww_mark = [&](uint32_t after) {
    if (e->d_lww_step0) hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_lww_step0, after);
  };
  // fused with dense-alone strict replays: the superstep that consumes host-staged tells runs eagerly
  // (block launch beside the dense launch): every bucket with staged tells would otherwise leave the
  // dense launch and void the replay
  bool eager_first = left && e->fused && e->stg_pending && e->dense_alone && dense_on(e, apply_variant(e));
  // staged host tells enter through an eager step (the graphs assume none)
  if (left && e->fused && e->stg_pending) {  // the next superstep consumes the staged tells
    e->stg_pending = false;
    e->hd_key.clear();
    e->hd_src.clear();
    e->hd_pay.clear();
  }
  if (left && e->n_staged_dev) {
    lww_mark(lww_next++);
    st = launch_step_single(e);
    --left;
  }
  const bool use_graph = !e->prof && e->graphs_enabled;
  bool strict = e->fused && use_graph && e->strict_ok;  // replays without skew launches (see d_abort)
  const uint32_t max_si = e->max_replay_si;
  auto size_idx = [&](uint32_t l) -> uint32_t {
    uint32_t si = l >= 16 ? 4u : l >= 8 ? 3u : l >= 4 ? 2u : l >= 2 ? 1u : 0u;
    return si < max_si ? si : max_si;
  };
  auto graph = [&](uint32_t si) -> hipGraphExec_t& {
    return e->fused ? e->gx[strict][e->par][si] : e->gx[0][e->par][si];
  };
  // every replay size (and, fused, both starting parities) is captured at first use, so no
  // capture ever lands in the middle of a later budget
  auto ensure_graphs = [&]() -> agx_status {
    if (!use_graph) return AGX_OK;
    const uint32_t p0 = e->par;  // capturing advances the host parity: restore it
    e->strict_cap = strict;
    agx_status s2 = AGX_OK;
    for (uint32_t p = 0; p < 2u && s2 == AGX_OK; ++p)  // (both starting parities: arenas are kernel arguments)
      for (uint32_t si = 0; si < agx_engine::kNSizes && s2 == AGX_OK; ++si) {
        hipGraphExec_t& g = e->fused ? e->gx[strict][p][si] : e->gx[0][p][si];
        if (g) continue;
        e->par = p;
        s2 = capture_steps(e, kGraphSizes[si], &g);
        (e->fused ? e->gx_persist[strict][p][si] : e->gx_persist[0][p][si]) = s2 == AGX_OK && e->captured_persist;
      }
    e->par = p0;
    e->strict_cap = false;
    return s2;
  };
  // agx_run(0): capture the replay graphs now (setup, like building the kernels), so that a run
  // timed from its first superstep -- bench.py's C3 tree -- does not pay ~10 graph captures inside
  // (the replays assume no host-staged chunk: a pending one is set aside for the capture -- the first
  // superstep of the next run consumes it eagerly, as always)
  if (max_steps == 0 && use_graph) {
    const uint32_t nsd = e->n_staged_dev;
    e->n_staged_dev = 0;
    const agx_status s2 = ensure_graphs();
    e->n_staged_dev = nsd;
    return s2;
  }
  // fused: per-superstep inbox sizes of each replay (pinned ring); the host counts the supersteps
  // with mail and stops at the first replay whose last superstep had none (quiescent)
  uint32_t rep_steps[kLag] = {0, 0, 0, 0};
  uint32_t rep_start[kLag] = {0, 0, 0, 0}, rep_par[kLag] = {0, 0, 0, 0};  // supersteps launched before it; parity
  bool rep_strict[kLag] = {false, false, false, false}, rep_void[kLag] = {false, false, false, false};
  const size_t ring_row = (size_t)agx_engine::kGraphSteps * e->nb + kRingTail;  // rows, 2 abort marks, the error word
  uint32_t rep_ring[kLag] = {0, 0, 0, 0};  // host ring slot of each replay in flight
  const uint32_t left0 = left;
  uint32_t launched_steps = 0;
  bool recovered = false;
  const uint32_t lww_run0 = lww_next;  // (the number the first superstep counted by launched_steps follows)
  int last_ring = -1;  // ring slot of the last fused replay launched (-1: eager work came last)
  auto fused_poll = [&](uint32_t slot) -> bool {
    const uint32_t* h = e->h_cntb + rep_ring[slot] * ring_row;
    bool last_empty = rep_steps[slot] > 0;
    for (uint32_t i = 0; i < rep_steps[slot]; ++i) {
      uint64_t t = 0;
      bool skew = false;  // a bucket's inbox over one LDS tile (it took the skew launch)
      bool tpend = false;  // timers: bit 31 of an entry = the bucket had a pending timer at the tick's entry
      for (uint32_t b = 0; b < e->nb; ++b) {
        uint32_t v = h[(size_t)i * e->nb + b];
        if (e->tm_keys || e->wd_slots) {  // (death watch: bit 31 = the stop rule held at the entry)
          tpend |= (v >> 31) != 0u;
          v &= 0x7FFFFFFFu;
        }
        t += v;
        skew |= v > (uint32_t)kBucket;
      }
      if (t) ++e->host_steps;
      e->clean_steps = skew ? 0u : e->clean_steps + 1u;
      last_empty = t == 0 && !tpend;
    }
    rep_steps[slot] = 0;
    return last_empty;
  };
  // A strict replay whose superstep k deferred a skewed bucket: supersteps after k (and every
  // replay launched after it) were no-ops.  Run k's skew launch, count k + 1 supersteps for this
  // replay, void the later ones, continue with the full graphs.
  // (A dense-alone strict replay -- k_dense_fused the whole superstep -- left its non-dense buckets
  // marked: k's block launch over the marks, then its skew launch; the strict graphs are recaptured
  // with the block launch from then on.)
  auto recover = [&](uint32_t slot, uint32_t k) -> agx_status {
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->par = rep_par[slot] ^ (k & 1u);
    e->cur_slot = k;
    const bool dense = e->dense_alone && dense_on(e, apply_variant(e));
    if (getenv("AGX_DEBUG_RECOVER")) {  // diagnostic: which buckets the aborting superstep left
      std::vector<uint32_t> bl(e->nb);
      if (dense) hipMemcpy(bl.data(), e->d_blist, e->nb * 4, hipMemcpyDeviceToHost);
      uint32_t nm = 0, first = ~0u;
      for (uint32_t b = 0; b < e->nb; ++b)
        if (bl[b]) {
          ++nm;
          if (first == ~0u) first = b;
        }
      fprintf(stderr, "[agx recover] replay slot %u superstep %u (launched %u): %s, %u buckets marked (first %u)\n", slot, k,
              rep_start[slot] + k, dense ? "dense-alone" : "skew", nm, first);
    }
    e->skew_only = !dense;
    e->recover_dense = dense;
    last_ring = -1;  // (eager launches after the replays: the error word is copied back)
    lww_mark(lww_run0 + rep_start[slot]);  // (superstep k of that replay again: cur_slot = k)
    lww_next = lww_run0 + rep_start[slot] + k + 1u;
    agx_status s2 = launch_apply(e, e->A);  // (advances e->par past superstep k)
    e->skew_only = false;
    e->recover_dense = false;
    e->cur_slot = 0;
    if (dense) {
      e->dense_alone = false;
      for (auto& a : e->gx[1])  // (strict graphs only: the replays in flight are full or void)
        for (auto& g : a) {
          if (g) hipGraphExecDestroy(g);
          g = nullptr;
        }
    }
    AGX_TRY(s2);
    HIP_TRY(hipMemcpyAsync(e->h_cntb + rep_ring[slot] * ring_row + (size_t)k * e->nb, e->d_cntb + (size_t)k * e->nb,
                           (size_t)e->nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_abort, 0, 8, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rep_steps[slot] = k + 1u;
    for (uint32_t q = 0; q < kLag; ++q)
      if (q != slot && rep_steps[q]) rep_void[q] = true;
    left = left0 - (rep_start[slot] + k + 1u);
    strict = false;
    e->strict_ok = false;
    recovered = true;
    return AGX_OK;
  };
  auto poll = [&](uint32_t slot) -> bool {  // true: quiescent
    if (rep_void[slot]) {
      rep_void[slot] = false;
      rep_steps[slot] = 0;
      return false;
    }
    if (rep_strict[slot] && rep_steps[slot]) {
      const uint32_t* ha = e->h_cntb + rep_ring[slot] * ring_row + agx_engine::kGraphSteps * e->nb;
      const uint32_t ab = ha[0] ? ha[0] : ha[1];
      if (ab) {
        const agx_status s2 = recover(slot, ab - 1u);
        if (s2 != AGX_OK) {
          st = s2;
          return true;
        }
      }
    }
    return fused_poll(slot);
  };
  uint32_t launched = 0;
  bool quiet = false;
  for (uint32_t it = 0; st == AGX_OK && left > 0; ++it) {
    const uint32_t slot = it % kLag;
    if (it >= kLag) {
      hipEventSynchronize(ev[slot]);
      if (e->fused) {
        if (poll(slot)) {
          quiet = true;
          break;
        }
        if (left == 0) break;  // (a recovery recounted the supersteps run)
        // two full replays without a skewed bucket: back to the strict graphs (a workload whose
        // skew was transient -- a Zipf burst -- regains the cheaper replays)
        if (!strict && use_graph && e->strict_env && e->clean_steps >= 2 * agx_engine::kGraphSteps) {
          strict = true;
          e->strict_ok = true;
        }
      } else if ((e->tm_keys || e->wd_slots) ? e->h_pin[8 + 2 * slot] != e->h_pin[9 + 2 * slot] : e->h_pin[slot] == 0) {
        // (timers: the last tick with mail or a pending timer at its entry is not that replay's last tick)
        break;  // that replay ended on a superstep with no mail: quiescent
      }
    }
    uint32_t cnt;
    const uint32_t par0 = e->par;
    const bool eager_now = eager_first;
    eager_first = false;
    lww_mark(lww_next);
    if (use_graph && eager_now) {  // one eager superstep, reported through the replay ring like a replay of 1
      cnt = 1;
      st = launch_step_single(e);
      if (st == AGX_OK)
        hipLaunchKernelGGL(k_replay_out, dim3(1), dim3(kScanThreads), 0, e->stream, e->d_cntb, e->nb, nullptr,
                           (const unsigned long long*)(e->d_stats + ST_ERROR), e->d_ring, e->d_rctr,
                           agx_engine::kGraphSteps * e->nb + kRingTail);
    } else if (use_graph) {
      st = ensure_graphs();
      if (st != AGX_OK) break;
      const uint32_t si = size_idx(left);
      cnt = kGraphSizes[si];
      hipError_t ge = hipGraphLaunch(graph(si), e->stream);
      if (ge != hipSuccess) {  // nothing ran: no parity, ring slot or replay-counter change
        st = set_err(AGX_EDEVICE, "hipGraphLaunch: %s", hipGetErrorString(ge));
        break;
      }
      if (cnt & 1u) e->par ^= 1u;  // the replayed supersteps advanced the parity
      if (e->fused && e->gx_persist[strict][par0][si]) {
        ++e->persist_launches;
        e->persist_supersteps += cnt;
      }
    } else {
      cnt = 1;
      st = launch_step_single(e);
    }
    left -= cnt;
    lww_next += cnt;
    ++launched;
    if (e->fused) {  // per-superstep inbox sizes of this replay
      rep_steps[slot] = cnt;
      rep_start[slot] = launched_steps;
      rep_par[slot] = par0;
      rep_strict[slot] = strict && !eager_now;
      rep_void[slot] = false;
      if (use_graph) {  // written by the graph's k_replay_out into ring slot (replay counter % kLag)
        rep_ring[slot] = (uint32_t)(e->replay_ctr++ % kLag);
        last_ring = (int)rep_ring[slot];
      } else {          // eager superstep: copied (the ring slots are all free between run_single calls)
        last_ring = -1;
        rep_ring[slot] = slot;
        uint32_t* hr = e->h_cntb + slot * ring_row;
        hipMemcpyAsync(hr, e->d_cntb, (size_t)cnt * e->nb * 4, hipMemcpyDeviceToHost, e->stream);
        hr[agx_engine::kGraphSteps * e->nb] = hr[agx_engine::kGraphSteps * e->nb + 1] = 0u;
      }
    } else {  // inbox total (sorted + backlog) of the replay's last superstep
      hipMemcpyAsync(&e->h_pin[slot], e->d_ninbox, 4, hipMemcpyDeviceToHost, e->stream);
      if (e->tm_keys) {  // the last active tick and the clock after this replay
        hipMemcpyAsync(&e->h_pin[8 + 2 * slot], e->d_timers + kTmLastAct, 4, hipMemcpyDeviceToHost, e->stream);
        hipMemcpyAsync(&e->h_pin[9 + 2 * slot], e->d_timers + kTmBucketOff + 2ull * e->nb, 4, hipMemcpyDeviceToHost, e->stream);
      }
      if (e->wd_slots) {  // (death watch: the same two words of its storage)
        hipMemcpyAsync(&e->h_pin[8 + 2 * slot], e->d_watch + kWdLastAct, 4, hipMemcpyDeviceToHost, e->stream);
        hipMemcpyAsync(&e->h_pin[9 + 2 * slot], e->d_watch + kWdBucketOff + 2ull * e->nb, 4, hipMemcpyDeviceToHost, e->stream);
      }
    }
    launched_steps += cnt;
    hipEventRecord(ev[slot], e->stream);
  }
  if (e->timing) {  // (agx_run_timed: after the last replay, before the sync)
    hipEventRecord(e->tev[1], e->stream);
    e->tev1_recorded = true;
  }
  // the kernels' error word rides on the final sync (agx_run checks it even when out == NULL): in the
  // last replay's ring row (k_replay_out) when a fused replay ended the run, else copied back
  if (last_ring < 0) hipMemcpyAsync(e->h_stat + ST_ERROR, e->d_stats + ST_ERROR, 8, hipMemcpyDeviceToHost, e->stream);
  hipStreamSynchronize(e->stream);
  if (last_ring >= 0) {
    const uint32_t* t = e->h_cntb + (size_t)last_ring * ring_row + ring_row - 2;
    e->h_stat[ST_ERROR] = (uint64_t)t[0] | ((uint64_t)t[1] << 32);
  }
  if ((e->h_stat[ST_ERROR] & kErrBarrier) && e->persist != 0) {  // (never again on this engine)
    e->persist = 0;
    drop_graphs(e);
  }
  const bool rec0 = recovered;
  if (e->fused && !quiet)  // replays not polled yet, in launch order
    for (uint32_t k = launched > kLag ? launched - kLag : 0; k < launched && st == AGX_OK; ++k)
      if (poll(k % kLag)) {
        quiet = true;
        break;
      }
  if (recovered && !rec0) {  // (a recovery above launched more work: its errors too)
    hipMemcpyAsync(e->h_stat + ST_ERROR, e->d_stats + ST_ERROR, 8, hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);
  }
  if (st == AGX_OK && recovered && !quiet && left > 0) return run_single(e, left);  // full graphs now
  return st;
}

// received state gossips -> rx rows (single kernel over the received range)
agx_status fix_rx(agx_engine* e, const Plan& p) {
  if (!e->pw || !p.n_recv) return AGX_OK;
  const uint32_t lo = (uint32_t)p.n_bl, hi = (uint32_t)(p.n_bl + p.n_recv);
  const uint32_t slo = (uint32_t)p.recv_off[e->rank], shi = (uint32_t)(p.recv_off[e->rank] + p.recv_cnt[e->rank]);
  hipLaunchKernelGGL(k_fix_rx, dim3(grid_for(p.n_recv / kThreads + 1, 2048)), dim3(kThreads), 0, e->stream, e->A.m(),
                     lo, hi, slo, shi, (uint32_t)e->heap_rows);
  HIP_TRY(hipGetLastError());
  return AGX_OK;
}

agx_status exchange_rccl(agx_engine* e, Plan& p) {
  // one contiguous (key, src, payload) run per peer: R sends instead of 3R (k_pack_aos / k_unpack_aos)
  hipLaunchKernelGGL(k_pack_aos, dim3(grid_for(e->cap_emit / kThreads + 1, 2048)), dim3(kThreads), 0, e->stream,
                     e->s2.c(), e->d_total, e->d_s2p);
  HIP_TRY(hipGetLastError());
  NCCL_TRY(ncclGroupStart());
  for (uint32_t q = 0; q < e->R; ++q) {
    if (p.send_cnt[q]) {
      const uint64_t o = p.send_off[q], n = p.send_cnt[q];
      NCCL_TRY(ncclSend(e->d_s2p + 3 * o, 3 * n, ncclUint32, (int)q, e->comm, e->stream));
      if (q != e->rank) {
        e->mr_sent_env += 12 * n;
        e->mr_sent_rows += 4ull * n * e->pw;
      }
      if (e->pw && q != e->rank)
        NCCL_TRY(ncclSend(e->d_s2rows + o * e->pw, n * e->pw, ncclUint32, (int)q, e->comm, e->stream));
    }
    if (p.recv_cnt[q]) {
      const uint64_t o = p.recv_off[q], n = p.recv_cnt[q];
      NCCL_TRY(ncclRecv(e->d_rcvp + 3 * (o - p.n_bl), 3 * n, ncclUint32, (int)q, e->comm, e->stream));
      if (e->pw && q != e->rank)
        NCCL_TRY(ncclRecv(e->d_rx + o * e->pw, n * e->pw, ncclUint32, (int)q, e->comm, e->stream));
    }
  }
  NCCL_TRY(ncclGroupEnd());
  if (p.n_recv) {  // received runs in sender-rank order after the local backlog (the sharded canonical order)
    hipLaunchKernelGGL(k_unpack_aos, dim3(grid_for(p.n_recv / kThreads + 1, 2048)), dim3(kThreads), 0, e->stream,
                       e->d_rcvp, (uint32_t)p.n_recv, e->A.m(), (uint32_t)p.n_bl);
    HIP_TRY(hipGetLastError());
  }
  return AGX_OK;
}

// ---- device-resident multi-rank supersteps (k_mr_pack / k_mr_unpack, agx_kernels.h)
// first slab: 17/16 of an even share of one superstep's tells per (sender, receiver) pair, + 1024
// (round 6; was 5/4): the wire bytes are slab-sized, and hash-sharded mail is even to within a few
// standard deviations (the 1M-per-rank ring: 125 K +- 0.35 K per pair at R = 8); skewed mail overflows
// once, takes the exact exchange for that superstep and grows the slabs to 5/4 of the largest count.
// Every rank must size it alike (the sends and receives are fixed-size): it depends on n_global,
// max_emit and R only, which the layout check compares (AGX_MR_SLAB overrides, on every rank).
uint32_t mr_initial_slab(const agx_engine* e) {
  if (const char* s = getenv("AGX_MR_SLAB")) return (uint32_t)std::max(1, atoi(s));
  const uint64_t share = e->n_global * e->kmax / ((uint64_t)e->R * e->R);
  return (uint32_t)std::min<uint64_t>(share + share / 16 + 1024, 1u << 30);
}

// (re)allocate the per-peer send / receive slabs (the same size on every rank: the decision to grow
// comes from the all-gathered counts, which every rank reads alike).  CRDT rows travel slab-sized
// too (R x slab rows of pw u32 to send and as many to receive): when they would leave the row handle
// space, pass the row budget (AGX_MR_ROW_MB, default 16384 MiB of the 288 GB HBM per rank) or fail
// to allocate on ANY rank -- all-gathered, so every rank decides alike -- every rank sets mr_host
// and runs the host-planned exchange (exact per-peer sizes) from then on.
agx_status mr_slabs(agx_engine* e, uint64_t want) {
  const uint32_t n = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 64), 1u << 30);
  if (n <= e->slab) return AGX_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  hipFree(e->d_sslab);
  hipFree(e->d_rslab);
  e->d_sslab = e->d_rslab = nullptr;
  e->slab = 0;
  drop_graphs(e);  // (the slabs are kernel and collective arguments of a captured replay)
  // this rank's verdict: 0 = the slabs fit, 1 = the envelope slabs fit but the CRDT row slabs do not
  // (host-planned exchange from now on), 2 = an allocation the exchange cannot do without failed.
  // No rank returns before the all-gather below: a rank that left early would leave its peers
  // blocked in the collective (every rank must take the same decision, from the same answers).
  uint64_t code = 0;
  if (dalloc(&e->d_sslab, (uint64_t)e->R * n * 3) != AGX_OK || dalloc(&e->d_rslab, (uint64_t)e->R * n * 3) != AGX_OK)
    code = 2;
  if (e->pw) {  // CRDT rows: row send slabs, and rx large enough to receive R slabs of rows
    const uint64_t rr = (uint64_t)e->R * n;
    const char* mb = getenv("AGX_MR_ROW_MB");
    const uint64_t budget = (mb ? (uint64_t)std::max(0, atoi(mb)) : 16384ull) << 20;
    hipFree(e->d_srows);
    e->d_srows = nullptr;
    bool fits = code == 0 && e->heap_rows + std::max<uint64_t>(rr, e->rx_rows) < kHandleMask &&
                2 * rr * e->pw * 4 <= budget;
    if (fits && dalloc_rows(&e->d_srows, rr * e->pw) != AGX_OK) fits = false;
    if (fits && rr > e->rx_rows) {
      hipFree(e->d_rx);
      e->d_rx = nullptr;
      if (dalloc_rows(&e->d_rx, rr * e->pw) == AGX_OK) {
        e->rx_rows = rr;
      } else {  // (the host-planned path needs rx of cap rows again)
        fits = false;
        e->rx_rows = 0;
        if (dalloc_rows(&e->d_rx, e->cap * e->pw) == AGX_OK)
          e->rx_rows = e->cap;
        else
          code = 2;
      }
    }
    if (!fits && code == 0) code = 1;
  }
  (void)hipGetLastError();  // (a refused allocation is an answer here, not an error)
  set_err(AGX_OK, "");
  // every rank's verdict (the exchange sizes must agree)
  e->h_pin64[0] = code;
  HIP_TRY(hipMemcpyAsync(e->d_cvec, e->h_pin64, 8, hipMemcpyHostToDevice, e->stream));
  NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, 1, ncclUint64, e->comm, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_pin64, e->d_cmat, (size_t)e->R * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  uint64_t worst = 0;
  for (uint32_t r = 0; r < e->R; ++r) worst = std::max<uint64_t>(worst, e->h_pin64[r]);
  if (worst >= 2) {  // every rank fails alike
    hipFree(e->d_sslab);
    hipFree(e->d_rslab);
    hipFree(e->d_srows);
    e->d_sslab = e->d_rslab = nullptr;
    e->d_srows = nullptr;
    return set_err(AGX_ENOMEM, "rank %u: exchange slabs of %u envelopes per peer could not be allocated on %s",
                   e->rank, n, code >= 2 ? "this rank" : "a peer rank");
  }
  if (worst == 1) {
    hipFree(e->d_srows);
    e->d_srows = nullptr;
    e->mr_host = true;
    if (getenv("AGX_MR_DEBUG"))
      fprintf(stderr, "[agx rank %u] CRDT row slabs of %u rows per peer do not fit on every rank: host-planned "
              "exchange\n", e->rank, n);
  }
  e->slab = n;
  return AGX_OK;
}

agx_status mr_step_dev(agx_engine* e, uint32_t idx);

// All-or-nothing capture: every rank all-gathers its capture result before the first replay, and a
// rank keeps its graph only if every rank captured -- otherwise all of them replay eagerly.  (A rank
// replaying its captured collectives while a peer issues the same collectives eagerly is legal for
// RCCL, but one rank's failed capture must not leave the ranks on different paths whose first
// launches then wait on each other.)
agx_status mr_agree_capture(agx_engine* e) {
  e->h_pin64[0] = e->mr_gx ? 1u : 0u;
  HIP_TRY(hipMemcpyAsync(e->d_cvec, e->h_pin64, 8, hipMemcpyHostToDevice, e->stream));
  NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, 1, ncclUint64, e->comm, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_pin64, e->d_cmat, (size_t)e->R * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  uint32_t ok = 0;
  for (uint32_t r = 0; r < e->R; ++r) ok += e->h_pin64[r] ? 1u : 0u;
  if (getenv("AGX_MR_DEBUG"))
    fprintf(stderr, "[agx rank %u] multi-rank replay capture: %u of %u ranks captured%s\n", e->rank, ok, e->R,
            ok == e->R ? "" : " -> eager replays on every rank");
  if (ok != e->R) {
    if (e->mr_gx) hipGraphExecDestroy(e->mr_gx);
    e->mr_gx = nullptr;
    e->mr_graph_ok = false;
  }
  return AGX_OK;
}

// kMrReplay device-resident supersteps as one graph.  A failed capture (a collective that cannot be
// captured) ends the capture, clears mr_graph_ok and returns AGX_OK: the caller replays eagerly.
agx_status capture_mr(agx_engine* e, uint32_t steps) {
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    e->mr_graph_ok = false;
    return AGX_OK;
  }
  agx_status st = AGX_OK;
  for (uint32_t i = 0; i < steps && st == AGX_OK; ++i) st = mr_step_dev(e, i);
  hipError_t ce = hipStreamEndCapture(e->stream, &g);
  hipGraphExec_t x = nullptr;
  if (st == AGX_OK && ce == hipSuccess && g && hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess &&
      hipGraphUpload(x, e->stream) == hipSuccess) {
    hipGraphDestroy(g);
    e->mr_gx = x;
    if (getenv("AGX_MR_DEBUG")) fprintf(stderr, "[agx rank %u] multi-rank replay captured (%u supersteps)\n", e->rank, steps);
    return AGX_OK;
  }
  if (getenv("AGX_MR_DEBUG"))
    fprintf(stderr, "[agx rank %u] multi-rank replay capture failed (status %d, %s): eager replays\n", e->rank, (int)st,
            hipGetErrorString(ce));
  if (x) hipGraphExecDestroy(x);
  if (g) hipGraphDestroy(g);
  (void)hipGetLastError();
  e->mr_graph_ok = false;
  set_err(AGX_OK, "");  // (the eager replays report their own errors)
  return AGX_OK;
}

// one superstep with no host round trip: phase 1, count all-gather, the decision and the send
// slabs (k_mr_pack), one fixed-size send / receive per peer, unpack, bucket passes, apply
agx_status mr_step_dev(agx_engine* e, uint32_t idx) {
  const uint32_t S = e->R + 2;
  const bool direct = e->pw == 0 && !getenv("AGX_MR_NO_DIRECT");  // (CRDT rows are laid out beside s2's tells)
  AGX_TRY(phase1(e, direct));
  MrArgs a{};
  a.cmat = e->d_cmat;
  a.s2 = e->s2.c();
  a.sslab = e->d_sslab;
  a.rslab = e->d_rslab;
  a.A = e->A.m();
  a.d_n = e->d_n;
  a.halt = e->d_halt;
  a.stats = e->d_stats;
  a.cap = e->cap;
  a.R = e->R;
  a.rank = e->rank;
  a.slab = e->slab;
  a.step = idx;
  a.s2rows = e->d_s2rows;
  a.srows = e->d_srows;
  a.pw = e->pw;
  a.heap_rows = (uint32_t)e->heap_rows;
  a.direct = direct ? 1u : 0u;
  e->mr_direct = direct;
  const dim3 g(grid_for((uint64_t)e->R * e->slab / kThreads + 1, 2048));
  {
    Scope sc(e, K_EXCHANGE);
    NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, S, ncclUint64, e->comm, e->stream));
    hipLaunchKernelGGL(k_mr_pack, g, dim3(kThreads), 0, e->stream, a);
    NCCL_TRY(ncclGroupStart());
    for (uint32_t q = 0; q < e->R; ++q) {
      if (q == e->rank) continue;
      NCCL_TRY(ncclSend(e->d_sslab + (size_t)q * e->slab * 3, 3ull * e->slab, ncclUint32, (int)q, e->comm, e->stream));
      NCCL_TRY(ncclRecv(e->d_rslab + (size_t)q * e->slab * 3, 3ull * e->slab, ncclUint32, (int)q, e->comm, e->stream));
      if (e->pw) {  // the state gossips' rows, slab-sized as well
        NCCL_TRY(ncclSend(e->d_srows + (size_t)q * e->slab * e->pw, (size_t)e->slab * e->pw, ncclUint32, (int)q, e->comm,
                          e->stream));
        NCCL_TRY(ncclRecv(e->d_rx + (size_t)q * e->slab * e->pw, (size_t)e->slab * e->pw, ncclUint32, (int)q, e->comm,
                          e->stream));
      }
    }
    NCCL_TRY(ncclGroupEnd());
    hipLaunchKernelGGL(k_mr_unpack, g, dim3(kThreads), 0, e->stream, a);
  }
  HIP_TRY(hipGetLastError());
  DevMsgs* sorted = nullptr;
  AGX_TRY(launch_bucket_sort(e, false, &sorted));
  return launch_apply(e, *sorted);
}

agx_status run_multi_rccl(agx_engine* e, uint32_t max_steps) {
  const uint32_t S = e->R + 2;
  Plan p;
  if (!e->layout_checked) {  // every rank must size rows and tells alike (same register_range / set_* calls):
                             // the send/recv sizes of the exchange are derived from them
    const uint64_t sig[2] = {((uint64_t)e->pw << 32) | e->delta_max, ((uint64_t)e->kmax << 32) | e->W};
    e->h_pin64[0] = sig[0];  // (pinned: the async copy reads it after this call returns)
    e->h_pin64[1] = sig[1];
    HIP_TRY(hipMemcpyAsync(e->d_cvec, e->h_pin64, 16, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, 2, ncclUint64, e->comm, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_pin64, e->d_cmat, (size_t)e->R * 16, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (uint32_t r = 0; r < e->R; ++r)
      if (e->h_pin64[2 * r] != sig[0] || e->h_pin64[2 * r + 1] != sig[1])
        return set_err(AGX_EINVAL, "rank %u and rank %u differ in row pitch / delta mode / max_emit / n_words "
                       "(make the same register_range and set_* calls on every rank)", e->rank, r);
    e->layout_checked = true;
  }
  // the host-planned exchange of a superstep whose phase 1 and count all-gather have run:
  // exact sizes from the count matrix (one host round trip); *quiet: nothing was in flight
  auto exact_rest = [&](bool* quiet) -> agx_status {
    HIP_TRY(hipMemcpyAsync(e->h_pin64, e->d_cmat, (size_t)e->R * S * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    make_plan(e, e->h_pin64, p);
    *quiet = p.total_inflight == 0;
    if (*quiet) return AGX_OK;
    if (p.n_bl + p.n_recv + p.n_staged > e->cap)
      return set_err(AGX_ECAPACITY, "rank %u: %llu messages in flight exceed capacity %llu", e->rank,
                     (unsigned long long)(p.n_bl + p.n_recv + p.n_staged), (unsigned long long)e->cap);
    {
      Scope sc(e, K_EXCHANGE);
      AGX_TRY(exchange_rccl(e, p));
    }
    AGX_TRY(fix_rx(e, p));
    return phase2(e, p.n_bl + p.n_recv + p.n_staged, p.n_bl + p.n_recv);
  };
  auto host_step = [&](bool* quiet) -> agx_status {
    AGX_TRY(phase1(e));
    {
      Scope sc(e, K_EXCHANGE);
      NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, S, ncclUint64, e->comm, e->stream));
    }
    return exact_rest(quiet);
  };
  uint32_t left = max_steps;
  bool quiet = false;
  // device-resident replays (CRDT rows travel in row slabs beside the envelope slabs); a staged
  // burst enters through one host-planned superstep (its staged count is a host number)
  const bool dev = !getenv("AGX_MR_HOST") && !e->mr_host;
  // whether ANY rank has staged tells: each rank knows only its own, and a rank that took the
  // host-planned superstep below while a peer went straight to the device replays would issue
  // different collectives than that peer (one all-gather per run, not per superstep)
  bool any_staged = e->n_staged_dev != 0;
  if (dev && left) {
    e->h_pin64[0] = e->n_staged_dev;
    HIP_TRY(hipMemcpyAsync(e->d_cvec, e->h_pin64, 8, hipMemcpyHostToDevice, e->stream));
    NCCL_TRY(ncclAllGather(e->d_cvec, e->d_cmat, 1, ncclUint64, e->comm, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_pin64, e->d_cmat, (size_t)e->R * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (uint32_t r = 0; r < e->R; ++r) any_staged = any_staged || e->h_pin64[r] != 0;
  }
  if (dev && any_staged && left) {
    AGX_TRY(host_step(&quiet));
    ++e->mr_host_steps;
    --left;
  }
  if (dev && !e->slab) AGX_TRY(mr_slabs(e, mr_initial_slab(e)));
  if (dev && !e->mr_host) {
    constexpr uint32_t kMrReplay = 8;  // supersteps enqueued before the host reads the stop word
    // kMrReplay supersteps captured as one graph (collectives included) and replayed: on by
    // default since round 5, AGX_MR_GRAPH=0 replays eagerly.  (Round 4 kept it opt-in after a run
    // "hung in its first launch"; the trace shows the replays completing and agx_destroy hanging in
    // ncclCommDestroy while the graph still held the communicator's persistent plans -- the graph
    // is now destroyed first, and the whole RCCL-rank suite passes with captured replays.)
    const char* mg = getenv("AGX_MR_GRAPH");
    const bool graphs = !e->prof && e->graphs_enabled && e->mr_graph_ok && (!mg || atoi(mg) != 0);
    while (left && !quiet && !e->mr_host) {
      const uint32_t k = std::min(left, kMrReplay);
      if (graphs && k == kMrReplay && !e->mr_gx) {
        AGX_TRY(capture_mr(e, kMrReplay));
        AGX_TRY(mr_agree_capture(e));
      }
      const bool dbg = getenv("AGX_MR_DEBUG") != nullptr;
      if (graphs && k == kMrReplay && e->mr_gx) {
        if (dbg) fprintf(stderr, "[agx rank %u] graph replay %llu: launch\n", e->rank, (unsigned long long)e->mr_replays);
        HIP_TRY(hipGraphLaunch(e->mr_gx, e->stream));
        ++e->mr_replays;
      } else {
        for (uint32_t i = 0; i < k; ++i) AGX_TRY(mr_step_dev(e, i));
      }
      HIP_TRY(hipMemcpyAsync(e->h_halt, e->d_halt, 8, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      const uint32_t code = e->h_halt[0], at = e->h_halt[1];
      if (dbg) fprintf(stderr, "[agx rank %u] %s of %u supersteps done: halt %u at %u\n", e->rank,
                       graphs && k == kMrReplay && e->mr_gx ? "graph replay" : "eager replay", k, code, at);
      const uint64_t sent = (uint64_t)(e->R - 1) * e->slab;  // fixed-size slabs per peer, per superstep
      if (!code) {
        left -= k;
        e->mr_dev_steps += k;
        e->mr_sent_env += k * 12 * sent;
        e->mr_sent_rows += k * 4 * sent * e->pw;
        continue;
      }
      left -= at;  // supersteps completed before the one that stopped (its phase 1 and all-gather ran)
      e->mr_dev_steps += at;
      e->mr_sent_env += at * 12 * sent;
      e->mr_sent_rows += at * 4 * sent * e->pw;
      HIP_TRY(hipMemsetAsync(e->d_halt, 0, 8, e->stream));
      if (code == 2u) break;  // nothing in flight (the host path's quiescence, same point)
      if (code == 3u)
        return set_err(AGX_ECAPACITY, "rank %u: messages in flight exceed capacity %llu", e->rank,
                       (unsigned long long)e->cap);
      // a sender -> receiver count over the slab: this superstep's exchange exactly, bigger slabs
      if (e->mr_direct) {  // (its peer runs went into the slabs: back into s2 for the exact exchange)
        hipLaunchKernelGGL(k_slab_to_s2, dim3(grid_for((uint64_t)e->R * e->slab / kThreads + 1, 2048)), dim3(kThreads), 0,
                           e->stream, (const uint64_t*)e->d_cmat, (const uint32_t*)e->d_sslab, e->s2.m(), e->R, e->rank,
                           e->slab);
        HIP_TRY(hipGetLastError());
      }
      AGX_TRY(exact_rest(&quiet));
      ++e->mr_exact;
      ++e->mr_host_steps;
      --left;
      uint64_t mx = 0;
      for (uint32_t r = 0; r < e->R; ++r)
        for (uint32_t q = 0; q < e->R; ++q)
          if (q != r) mx = std::max<uint64_t>(mx, e->h_pin64[r * S + q]);
      AGX_TRY(mr_slabs(e, mx + mx / 4 + 1024));
    }
  }
  // host-planned supersteps: AGX_MR_HOST, or CRDT row slabs that do not fit (mr_slabs)
  for (; left && !quiet; --left) {
    AGX_TRY(host_step(&quiet));
    ++e->mr_host_steps;
  }
  HIP_TRY(hipMemcpyAsync(e->h_stat + ST_ERROR, e->d_stats + ST_ERROR, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return AGX_OK;
}

void drop_graphs(agx_engine* e) {
  if (e->mr_gx && getenv("AGX_MR_DEBUG")) fprintf(stderr, "[agx rank %u] multi-rank replay graph dropped\n", e->rank);
  for (auto& a : e->gx)
    for (auto& b : a)
      for (auto& g : b) {
        if (g) hipGraphExecDestroy(g);
        g = nullptr;
      }
  if (e->mr_gx) hipGraphExecDestroy(e->mr_gx);
  e->mr_gx = nullptr;
}

// First CRDT kind (or a wider one): size the snapshot heap for `kind`'s rows (full state, plus
// deltaVersions and DeltaPropagation rows in delta-CRDT mode; include/akka_gpu.h).
agx_status enable_crdt(agx_engine* e, uint32_t kind) {
  static_assert((2 * AGX_LWWMAP_WORDS + kRowAlign - 1) / kRowAlign * kRowAlign >= kLwRowMax,
                "the row pitch of an LWWMap engine holds the widest LWWMap snapshot row (agx_lwwmap.h)");
  static_assert((2 * AGX_PNCMAP_WORDS + kRowAlign - 1) / kRowAlign * kRowAlign >= kPnRowMax && kPnRowMax == 2592u,
                "the row pitch of a PNCounterMap engine holds the widest PNCounterMap snapshot row (agx_pncmap.h)");
  static_assert(AGX_PNCMAP_WORDS == 1296u && AGX_PNCMAP_WORDS % 16u == 0 && AGX_PNCMAP_WORDS <= AGX_MAX_WORDS,
                "a PNCounterMap state is 81 lines of 128 B: the actor-major pitch (prepare_run) is exact");
  static_assert((2 * AGX_ORMM_WORDS + kRowAlign - 1) / kRowAlign * kRowAlign == kMmRowMax && kMmRowMax == 5152u,
                "the row pitch of an ORMultiMap engine is exactly the widest ORMultiMap snapshot row (agx_ormm.h)");
  static_assert(AGX_ORMM_WORDS == 2576u && AGX_ORMM_WORDS % 16u == 0 && AGX_ORMM_WORDS <= AGX_MAX_WORDS,
                "an ORMultiMap state is 161 lines of 128 B: the actor-major pitch (prepare_run) is exact");
  if (kind == AGX_KIND_ORMULTIMAP && e->delta_max)
    return set_err(AGX_EINVAL, "ORMultiMap replicas gossip their full state: not on an engine with delta-CRDT "
                   "replication (agx_set_delta_crdt; ORMap delta ops are left out)");
  if (kind == AGX_KIND_ORMULTIMAP && e->W != AGX_ORMM_WORDS)
    return set_err(AGX_EINVAL, "ORMultiMap replicas need an engine with n_words = %u (got %u)", AGX_ORMM_WORDS, e->W);
  if (kind == AGX_KIND_PNCOUNTERMAP && e->delta_max)
    return set_err(AGX_EINVAL, "PNCounterMap replicas gossip their full state: not on an engine with delta-CRDT "
                   "replication (agx_set_delta_crdt; ORMap delta ops are left out)");
  if (kind == AGX_KIND_LWWMAP && e->delta_max)
    return set_err(AGX_EINVAL, "LWWMap replicas gossip their full state: not on an engine with delta-CRDT replication "
                   "(agx_set_delta_crdt; ORMap delta ops are left out)");
  const uint32_t words = kind == AGX_KIND_GCOUNTER ? AGX_GCOUNTER_WORDS
                         : kind == AGX_KIND_PNCOUNTER ? AGX_PNCOUNTER_WORDS
                         : kind == AGX_KIND_LWWMAP ? AGX_LWWMAP_WORDS
                         : kind == AGX_KIND_PNCOUNTERMAP ? AGX_PNCMAP_WORDS
                         : kind == AGX_KIND_ORMULTIMAP ? AGX_ORMM_WORDS : AGX_ORSET_WORDS;
  const uint32_t need = !e->delta_max ? words
                        : kind == AGX_KIND_GCOUNTER ? AGX_GCOUNTER_DELTA_WORDS
                        : kind == AGX_KIND_PNCOUNTER ? AGX_PNCOUNTER_DELTA_WORDS : AGX_ORSET_DELTA_WORDS;
  if (e->W < need) return set_err(AGX_EINVAL, "behaviour kind %u needs n_words >= %u", kind, need);
  const uint32_t ru = !e->delta_max ? 2 * words : kind == AGX_KIND_ORSET ? AGX_ORSET_DELTA_ROW_U32
                                                                          : 2 * words + AGX_CRDT_NODES;
  // row pitch in u32: rows wider than one 128-B line start on a line boundary (ORSet: 2080 B
  // rows padded to 2176 B), so a merge's batched row loads never split a line between rows
  const uint32_t pw = ru > kRowAlign ? (ru + kRowAlign - 1) / kRowAlign * kRowAlign : ru;
  if (pw <= e->pw) return AGX_OK;
  if (e->started) return set_err(AGX_ESTATE, "register CRDT kinds before the first agx_run");
  if (const Feature f = active_feature(e); f != F_NONE)
    return set_err(AGX_EINVAL, "CRDT kinds cannot be registered on an engine with %s%s", kFeatures[f].crdt_named,
                   kFeatures[f].crdt_why);
  const uint64_t rows = ((uint64_t)e->nb << e->bb) + e->cap;
  if (rows + e->cap > kHandleMask) return set_err(AGX_EINVAL, "CRDT kinds need msg_capacity < 2^28 - n_actors");
  hipFree(e->d_heap);
  hipFree(e->d_rx);
  hipFree(e->d_s2rows);
  e->d_heap = e->d_rx = e->d_s2rows = nullptr;
  e->pw = 0;
  AGX_TRY(dalloc_rows(&e->d_heap, 2 * rows * pw));
  e->heap_rows = rows;
  if (e->R > 1) {
    AGX_TRY(dalloc_rows(&e->d_rx, e->cap * pw));
    AGX_TRY(dalloc_rows(&e->d_s2rows, e->cap_emit * pw));
    e->rx_rows = e->cap;
    hipFree(e->d_srows);
    e->d_srows = nullptr;
    e->slab = 0;  // (the row slabs are sized with the envelope slabs, for this pitch)
  }
  e->pw = pw;
  drop_graphs(e);
  return AGX_OK;
}

agx_status validate_cfg(const agx_cfg* c) {
  if (!c) return set_err(AGX_EINVAL, "null cfg");
  if (c->abi_version != AGX_ABI_VERSION) return set_err(AGX_EINVAL, "abi_version %u != %u", c->abi_version, AGX_ABI_VERSION);
  if (c->n_actors == 0 || c->n_actors >= (1ull << 31)) return set_err(AGX_EINVAL, "n_actors out of range");
  // every layout but an ORMultiMap replica's fits AGX_MAX_GENERAL_WORDS; the widths between that and
  // AGX_ORMM_WORDS belong to no kind (an ORMultiMap engine takes exactly AGX_ORMM_WORDS: enable_crdt)
  static_assert(AGX_MAX_GENERAL_WORDS == AGX_PNCMAP_WORDS && AGX_MAX_WORDS == AGX_ORMM_WORDS && AGX_MAX_GENERAL_WORDS < AGX_MAX_WORDS,
                "n_words: 1..AGX_MAX_GENERAL_WORDS, or AGX_MAX_WORDS for an ORMultiMap engine");
  if (c->n_words == 0 || (c->n_words > AGX_MAX_GENERAL_WORDS && c->n_words != AGX_MAX_WORDS))
    return set_err(AGX_EINVAL, "n_words must be 1..%u, or %u for an engine of ORMultiMap replicas", AGX_MAX_GENERAL_WORDS,
                   AGX_MAX_WORDS);
  uint32_t R = c->n_ranks ? c->n_ranks : 1;
  if (R > AGX_MAX_RANKS || c->rank >= R) return set_err(AGX_EINVAL, "bad rank %u / n_ranks %u", c->rank, R);
  if (c->num_shards > (uint32_t)INT32_MAX) return set_err(AGX_EINVAL, "num_shards must be < 2^31 (maxNumberOfShards is an Int)");
  const uint32_t ba = c->bucket_actors;
  if (ba && (ba & (ba - 1) || ba < (1u << kMinBucketBits) || ba > (uint32_t)kBucket))
    return set_err(AGX_EINVAL, "bucket_actors must be 0 or a power of two in [%d, %d]", 1 << kMinBucketBits, kBucket);
  return AGX_OK;
}

}  // namespace

// =========================================================================
// C ABI
// =========================================================================
extern "C" {

const char* agx_last_error(void) { return g_err.c_str(); }
uint32_t agx_abi_version(void) { return AGX_ABI_VERSION; }

// The source hash this library was built from (__graft_entry__.source_hash, passed by build_native);
// the stamp is found in the file's bytes without loading it, so a stale library is rebuilt.
#ifndef AGX_BUILD_HASH
#define AGX_BUILD_HASH "unstamped000000"
#endif
extern "C" __attribute__((used, visibility("default"))) const char agx_build_stamp[] = "AGX_BUILD_HASH=" AGX_BUILD_HASH;
const char* agx_build_hash(void) { return agx_build_stamp + 15; }

int32_t agx_shard_id(uint32_t id, uint32_t num_shards) {
  if (num_shards == 0 || num_shards > (uint32_t)INT32_MAX) return 0;  // (maxNumberOfShards is an Int)
  int32_t h = java_hash_decimal(id);
  int32_t a = (h == INT32_MIN) ? INT32_MIN : (h < 0 ? -h : h);  // math.abs(Int.MinValue) stays negative
  return a % (int32_t)num_shards;
}

uint32_t agx_owner(uint32_t id, uint32_t num_shards, uint32_t n_ranks) {
  if (n_ranks <= 1) return 0;
  int32_t m = agx_shard_id(id, num_shards) % (int32_t)n_ranks;
  return (uint32_t)(m < 0 ? m + (int32_t)n_ranks : m);
}

agx_status agx_create(const agx_cfg* cfg, agx_engine** out) {
  AGX_TRY(validate_cfg(cfg));
  if (!out) return set_err(AGX_EINVAL, "null out");
  auto* e = new agx_engine();
  e->cfg = *cfg;
  e->n_global = cfg->n_actors;
  e->T = cfg->throughput == 0 || (int32_t)cfg->throughput < 0 ? 1u : cfg->throughput;  // Mailbox.scala:261
  e->Traw = e->T;
  e->C = cfg->capacity;
  e->mcap[0] = e->C;
  if (e->C && e->T > e->C) e->T = e->C;  // a bounded queue never holds more than C: drain <= min(T, C)
  e->W = cfg->n_words;
  e->kmax = std::max<uint32_t>(1, cfg->max_emit);
  e->R = cfg->n_ranks ? cfg->n_ranks : 1;
  e->rank = cfg->rank;
  e->num_shards = cfg->num_shards ? cfg->num_shards : 1000;
  e->bb = cfg->bucket_actors ? ceil_log2(cfg->bucket_actors) : (uint32_t)kBucketBits;
  if (const char* s = getenv("AGX_TINY")) e->tiny_max = std::min<uint32_t>(kTinyMax, (uint32_t)std::max(0, atoi(s)));
  if (const char* s = getenv("AGX_TINY_LAUNCH")) e->tiny_launch = atoi(s) != 0;
  if (const char* s = getenv("AGX_DENSE_LAUNCH")) e->dense_launch = atoi(s) != 0 ? 1 : 0;
  if (const char* s = getenv("AGX_DENSE_FUSED")) e->dense_fused = atoi(s) != 0;
  if (const char* s = getenv("AGX_DENSE_OWNER")) e->dense_owner = atoi(s) != 0;
  if (const char* s = getenv("AGX_BUCKET_ACTORS")) {  // diagnostic: override the bucket width (power of two)
    const uint32_t ba = (uint32_t)atoi(s);
    if (ba >= (1u << kMinBucketBits) && ba <= (uint32_t)kBucket && !(ba & (ba - 1))) e->bb = ceil_log2(ba);
  }
  e->graphs_enabled = getenv("AGX_NO_GRAPH") == nullptr && getenv("AGX_STAMPS") == nullptr;
  agx_status st = ensure_dev(e);
  if (st) { delete e; return st; }

  // ShardRegion hash sharding: owner(id) = floor-mod(shardId(id), R); local index = rank among owned ids
  if (e->R > 1) {
    e->h_route.resize(e->n_global);
    uint64_t nl = 0;
    std::vector<uint32_t> cnt(e->R, 0);
    for (uint64_t id = 0; id < e->n_global; ++id) {
      uint32_t o = agx_owner((uint32_t)id, e->num_shards, e->R);
      e->h_route[id] = (o << kOwnerShift) | cnt[o];
      if (o == e->rank) e->h_gid.push_back((uint32_t)id);
      cnt[o]++;
    }
    nl = cnt[e->rank];
    for (uint32_t o = 0; o < e->R; ++o)
      if (cnt[o] > kLocalMask) { delete e; return set_err(AGX_EINVAL, "too many actors per rank"); }
    e->n_local = nl;
  } else {
    if (e->n_global > kLocalMask) { delete e; return set_err(AGX_EINVAL, "n_actors exceeds 2^28 per rank"); }
    e->n_local = e->n_global;
  }
  const uint64_t nl = std::max<uint64_t>(e->n_local, 1);
  e->key_bits = std::max<uint32_t>(1, ceil_log2(nl));
  e->cap = cfg->msg_capacity ? cfg->msg_capacity : std::max<uint64_t>(4 * nl, 1u << 16);
  if (e->cap >= (1ull << 32) - kTile) { delete e; return set_err(AGX_EINVAL, "msg_capacity too large"); }
  e->cap_emit = e->cap * e->kmax;  // bucket b's tells live at [lo*kmax, (lo+cnt)*kmax)
  if (e->cap_emit >= (1ull << 32)) { delete e; return set_err(AGX_EINVAL, "msg_capacity * max_emit must be < 2^32"); }
  {  // largest super-tile of the dense sort passes: about 1024+ workgroups at full capacity; each pass
     // picks its own size from its input (pass_super), down to one tile, so the histogram table is
     // sized for one-tile super-tiles
    const uint64_t mx = std::max(e->cap, e->cap_emit);
    e->dsub = (uint32_t)std::min<uint64_t>(kSub, std::max<uint64_t>(1, mx / ((uint64_t)kTile * 1024)));
  }
  e->max_supers = (uint32_t)((std::max(e->cap, e->cap_emit) + kTile - 1) / kTile + 1);
  e->dstride = (e->max_supers + 3) & ~3u;
  // buckets of 2^bb actors; LSD passes over key bits [bb, key_bits), <= kRadixBits each
  e->nb = (uint32_t)((nl + (1ull << e->bb) - 1) >> e->bb);
  e->nchunks = 2 * e->nb + kStagedChunks;
  // first-pass histogram columns: ~2048 units per arena at most (G buckets per unit)
  e->G = (e->nb + 2047) / 2048;
  if (const char* s = getenv("AGX_UNIT_G")) e->G = (uint32_t)std::max(1, atoi(s));  // test knob
  e->G = std::min<uint32_t>(e->G, kMaxUnitChunks);
  e->ng = (e->nb + e->G - 1) / e->G;
  e->nunits = 2 * e->ng + kStagedChunks;
  e->cstride = (e->nunits + 3) & ~3u;
  {
    const uint32_t lo = e->bb, hi = std::max<uint32_t>(e->key_bits, e->bb + 1);
    // AGX_RADIX_BITS (test knob): narrower digits, so that small populations take the multi-pass path
    uint32_t rb = kRadixBits;
    if (const char* s = getenv("AGX_RADIX_BITS")) rb = std::min<uint32_t>(kRadixBits, std::max(1, atoi(s)));
    e->plan.npass = (hi - lo + rb - 1) / rb;
    if (e->plan.npass > 4) { delete e; return set_err(AGX_EINVAL, "AGX_RADIX_BITS=%u needs more than 4 passes", rb); }
    for (uint32_t p = 0, sh = lo; p < e->plan.npass; ++p) {
      const uint32_t b = (hi - sh + (e->plan.npass - p) - 1) / (e->plan.npass - p);  // spread bits evenly
      e->plan.shift[p] = sh;
      e->plan.bits[p] = b;
      sh += b;
    }
    // AGX_PASS0_BITS (A/B knob): the first (chunk-list) pass's digit width, the rest spread over the
    // dense passes -- fewer first-pass digits make longer per-digit runs out of its small tiles
    if (const char* s = getenv("AGX_PASS0_BITS"); s && e->plan.npass > 1) {
      const uint32_t b0 = std::min<uint32_t>(rb, std::max(1, atoi(s)));
      if (b0 < hi - lo) {
        const uint32_t rest = hi - lo - b0, np = (rest + rb - 1) / rb;
        if (1 + np <= 4) {
          e->plan.npass = 1 + np;
          e->plan.shift[0] = lo;
          e->plan.bits[0] = b0;
          for (uint32_t p = 1, sh = lo + b0; p < e->plan.npass; ++p) {
            const uint32_t b = (hi - sh + (e->plan.npass - p) - 1) / (e->plan.npass - p);
            e->plan.shift[p] = sh;
            e->plan.bits[p] = b;
            sh += b;
          }
        }
      }
    }
  }

  // fused superstep when one radix digit covers every bucket of a single rank
  e->fused = e->R == 1 && e->plan.npass == 1 && getenv("AGX_NO_FUSED") == nullptr;
  // identity grouping (k_ident_combine): single-rank multi-pass with a bucket-bounds search
  e->ident_on = !e->fused && e->R == 1 && e->plan.npass > 1 && getenv("AGX_NO_IDENT") == nullptr;
  if (!e->fused && e->R == 1) e->par = 1u;  // multi-pass: parity of the first superstep's counter value (1)
  e->tstride = (e->nb + 3) & ~3u;
  // fused: bucket b's inbox (and its backlog / tell slices) live at [b*region, ...) of the
  // arenas; an inbox larger than the region (skew) takes a slot of the overflow area that
  // follows, sized like the whole message capacity — no shared counter on the common path
  e->region = kBucket;
  if (getenv("AGX_NO_STRICT")) e->strict_ok = e->strict_env = false;
  if (const char* s = getenv("AGX_MAX_REPLAY")) {  // diagnostic: cap the replay length (1, 2, 4, 8)
    const uint32_t m = (uint32_t)std::max(1, atoi(s));
    e->max_replay_si = m >= 16 ? 4u : m >= 8 ? 3u : m >= 4 ? 2u : m >= 2 ? 1u : 0u;
  }
  e->stamps_skew = getenv("AGX_STAMPS_SKEW") != nullptr;
  if (const char* s = getenv("AGX_SKEW_GRID"))
    e->skew_grid = (uint32_t)std::min<int>(kMaxApplyGrid, std::max(1, atoi(s)));
  if (const char* s = getenv("AGX_APPLY_GRID"))
    e->apply_grid = (uint32_t)std::min<int>(kMaxApplyGrid, std::max(1, atoi(s)));
  e->acap = e->fused ? (uint64_t)e->nb * e->region + e->cap : e->cap;
  if (e->acap * e->kmax >= (1ull << 32)) { delete e; return set_err(AGX_EINVAL, "msg_capacity * max_emit too large"); }
  // bounded-mailbox rings: drain scratch / tell slices of kBucket x throughput messages per pool slot
  // after the arenas (AGX_RING_SLOTS: how many; CRDT kinds are registered later and turn the pool off
  // at the first run; class 0 is agx_cfg.capacity, so an unbounded default never has rings).
  // Opt-in: measured same-box against the backlog arena they cost C5 -2 % and C3 -6 % (every ring
  // bucket takes the four-kernel skew path each superstep)
  if (!e->fused && e->R == 1 && e->Traw <= kRingMaxT && e->mcap[0] && e->mcap[0] <= kRingMaxC) {
    uint64_t want = 0;
    if (const char* s = getenv("AGX_RING_SLOTS")) want = (uint64_t)std::max(0, atoi(s));
    const uint64_t per = (uint64_t)kBucket * e->Traw;
    const uint64_t room = ((1ull << 32) / e->kmax - 1 - e->acap) / per;
    e->ring_res = (uint32_t)std::min<uint64_t>({want, e->nb, room});
  }
  const uint64_t ring_extra = (uint64_t)e->ring_res * kBucket * e->Traw;

  e->h_kind.assign(e->n_local, 0);
  e->h_alive.assign(e->n_local, 0);
  e->h_state.assign(e->n_local * e->W, 0);

#define CREATE_TRY(x)            \
  do {                           \
    agx_status _s = (x);         \
    if (_s) { agx_destroy(e); return _s; } \
  } while (0)
  CREATE_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess
                 ? AGX_OK
                 : set_err(AGX_EDEVICE, "hipStreamCreate failed"));
  CREATE_TRY(dalloc(&e->d_kind, nl));
  // (padded to whole buckets: the apply loads every bucket's flags as u32 words, masked past n_local)
  const uint64_t alive_sz = ((uint64_t)e->nb << e->bb) + kBucket + 64;
  CREATE_TRY(dalloc(&e->d_alive, alive_sz));
  CREATE_TRY(hipMemset(e->d_alive, 0, alive_sz) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_stopq, nl));
  CREATE_TRY(dalloc(&e->d_nstop, 4));
  CREATE_TRY(hipMemset(e->d_nstop, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_state, nl * e->W));
  // two-word engines (the plain behaviours' count + cursor / sum): actor-major pairs on the device
  // (DevParams::sa / sw; the host mirror stays word-major, transposed at upload / read-back).
  // A CRDT kind needs n_words >= 8, so a two-word engine never becomes a CRDT engine.
  if (e->W == 2 && !getenv("AGX_STATE_SOA")) e->pitch = 2;
  if (e->R > 1) {
    CREATE_TRY(dalloc(&e->d_gid, nl));
    CREATE_TRY(dalloc(&e->d_route, e->n_global));
    CREATE_TRY(hipMemcpy(e->d_gid, e->h_gid.data(), e->n_local * 4, hipMemcpyHostToDevice) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "upload gid"));
    CREATE_TRY(hipMemcpy(e->d_route, e->h_route.data(), e->n_global * 4, hipMemcpyHostToDevice) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "upload route"));
  }
  CREATE_TRY(alloc_msgs(e->A, e->acap));
  CREATE_TRY(alloc_msgs(e->B, e->fused ? 1 : e->cap));
  CREATE_TRY(alloc_msgs(e->scr, e->acap + ring_extra));
  CREATE_TRY(alloc_msgs(e->bl, e->acap));
  e->em_cap = (e->acap + ring_extra) * e->kmax;
  CREATE_TRY(alloc_msgs(e->em, e->em_cap));
  if (e->R > 1) {  // tells grouped by owner per bucket (eg0 + [R][tstride] tables), send buffer s2
    const uint64_t tsz = (uint64_t)e->R * e->tstride;
    CREATE_TRY(alloc_msgs(e->eg0, e->cap_emit));
    CREATE_TRY(alloc_msgs(e->s2, e->cap_emit));
    CREATE_TRY(dalloc(&e->d_s2p, 3 * e->cap_emit));
    CREATE_TRY(dalloc(&e->d_rcvp, 3 * e->cap));
    CREATE_TRY(dalloc(&e->d_halt, 2));
    CREATE_TRY(hipMemset(e->d_halt, 0, 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(hipHostMalloc((void**)&e->h_halt, 8, hipHostMallocDefault) == hipSuccess ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
    CREATE_TRY(dalloc(&e->d_tcnt[0], tsz));
    CREATE_TRY(dalloc(&e->d_toff[0], tsz));
    CREATE_TRY(hipMemset(e->d_tcnt[0], 0, tsz * 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(dalloc(&e->d_moff0, e->nb));
    CREATE_TRY(dalloc(&e->d_moff1, tsz));
  }
  if (!e->fused && e->R == 1) {  // multi-pass: backlog and tell arenas by superstep parity
    CREATE_TRY(alloc_msgs(e->bl2, e->acap));
    CREATE_TRY(alloc_msgs(e->em2, e->em_cap));
    if (e->ident_on) {
      CREATE_TRY(dalloc(&e->d_emmeta, e->nb));
      CREATE_TRY(dalloc(&e->d_slsum, (uint64_t)(kMaxBlSlices + 1) * kSlSum));
      CREATE_TRY(dalloc(&e->d_ident, 4));
      CREATE_TRY(hipMemset(e->d_emmeta, 0, e->nb * sizeof(uint4)) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
      CREATE_TRY(hipMemset(e->d_ident, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    }
    CREATE_TRY(dalloc(&e->d_blpre, e->nb + 2 * kMaxBlSlices));  // [nb] prefixes, [64] slice totals, [64] bases
    CREATE_TRY(dalloc(&e->d_ninbox, 1));
    CREATE_TRY(hipMemset(e->d_ninbox, 0, 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    // skewed-bucket partitions: a skewed bucket holds > kBucket messages, so at most cap / kBucket
    // of them; parts of >= kSkSpan positions.  k_skew_plan rounds a bucket's backlog parts and its
    // new-mail parts up separately, so each skewed bucket adds up to TWO parts beyond the budget:
    // at most sk_budget + 2 x (skewed buckets) rows of pc
    const uint64_t nsk = std::min<uint64_t>(e->nb, e->cap / kBucket + 1);
    e->sk_budget = (uint32_t)std::min<uint64_t>(8192, e->cap / kSkSpan + 1);
    e->sk_rows = e->sk_budget + 2 * (uint32_t)nsk;
    CREATE_TRY(dalloc(&e->d_sk_rec, (uint64_t)e->nb * kSkRec));
    CREATE_TRY(dalloc(&e->d_sk_act, nsk * kSkActPlanes * kBucket));
    CREATE_TRY(dalloc(&e->d_sk_pc, (uint64_t)e->sk_rows * kBucket));
    CREATE_TRY(dalloc(&e->d_sk_meta, 4));
  }
  if (e->fused) {
    const uint64_t tsz = (uint64_t)kRadix * e->tstride;
    CREATE_TRY(alloc_msgs(e->bl2, e->acap));
    CREATE_TRY(alloc_msgs(e->eg0, e->acap * e->kmax));
    CREATE_TRY(alloc_msgs(e->eg1, e->acap * e->kmax));
    for (int q = 0; q < 2; ++q) {
      CREATE_TRY(dalloc(&e->d_tcnt[q], tsz));
      CREATE_TRY(dalloc(&e->d_toff[q], tsz));
      CREATE_TRY(dalloc(&e->d_blo[q], e->nb));
      CREATE_TRY(dalloc(&e->d_blc[q], e->nb));
      CREATE_TRY(dalloc(&e->d_emc[q], e->nb));
      CREATE_TRY(hipMemset(e->d_tcnt[q], 0, tsz * 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
      CREATE_TRY(hipMemset(e->d_blc[q], 0, e->nb * 4ull) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
      CREATE_TRY(hipMemset(e->d_emc[q], 0, e->nb * 4ull) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    }
    CREATE_TRY(dalloc(&e->d_stg_off, e->nb));
    CREATE_TRY(dalloc(&e->d_stg_cnt, e->nb));
    CREATE_TRY(dalloc(&e->d_ovf, 2));
    CREATE_TRY(dalloc(&e->d_cntb, (uint64_t)agx_engine::kGraphSteps * e->nb));
    CREATE_TRY(hipHostMalloc((void**)&e->h_cntb, 4ull * (agx_engine::kGraphSteps * e->nb + kRingTail) * 4, hipHostMallocDefault) ==
                       hipSuccess ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
    CREATE_TRY(dalloc(&e->d_parv, 2));
    const uint32_t parv[2] = {0u, 1u};
    CREATE_TRY(hipMemcpy(e->d_parv, parv, 8, hipMemcpyHostToDevice) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "upload"));
    CREATE_TRY(hipMemset(e->d_stg_cnt, 0, e->nb * 4ull) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(hipMemset(e->d_ovf, 0, 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(hipHostGetDevicePointer((void**)&e->d_ring, e->h_cntb, 0) == hipSuccess ? AGX_OK
                   : set_err(AGX_EDEVICE, "hipHostGetDevicePointer"));
    CREATE_TRY(dalloc(&e->d_rctr, 1));
    CREATE_TRY(hipMemset(e->d_rctr, 0, 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(dalloc(&e->d_abort, 2));
    CREATE_TRY(hipMemset(e->d_abort, 0, 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(dalloc(&e->d_pbar, 4));
    CREATE_TRY(hipMemset(e->d_pbar, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
    CREATE_TRY(hipHostMalloc((void**)&e->h_abort, 4 * 2 * 4, hipHostMallocDefault) == hipSuccess
                   ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
  }
  CREATE_TRY(dalloc(&e->d_skew_list, e->nb));
  CREATE_TRY(dalloc(&e->d_skew_n, 4));
  CREATE_TRY(hipMemset(e->d_skew_n, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_blist, e->nb));
  CREATE_TRY(dalloc(&e->d_dense_left, 2));
  CREATE_TRY(hipMemset(e->d_dense_left, 0, 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_chunk_off, e->nchunks));
  CREATE_TRY(dalloc(&e->d_chunk_cnt, e->nchunks));
  CREATE_TRY(hipMemset(e->d_chunk_off, 0, e->nchunks * 4ull) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(hipMemset(e->d_chunk_cnt, 0, e->nchunks * 4ull) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_hist_c, (uint64_t)kRadix * e->cstride));
  CREATE_TRY(hipMemset(e->d_hist_c, 0, (uint64_t)kRadix * e->cstride * 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_bstart, std::max<uint64_t>(kRadix, e->nb) + 1));
  if (getenv("AGX_STAMPS")) {
    CREATE_TRY(dalloc(&e->d_dbg, (uint64_t)std::min<uint64_t>(e->nb, 4096) * 16));
    CREATE_TRY(hipMemset(e->d_dbg, 0, std::min<uint64_t>(e->nb, 4096) * 16 * 8) == hipSuccess ? AGX_OK
                                                                                       : set_err(AGX_EDEVICE, "memset"));
  }
  CREATE_TRY(dalloc(&e->d_hist_d, (uint64_t)kRadix * e->dstride));
  CREATE_TRY(dalloc(&e->d_tot, kRadix));
  CREATE_TRY(dalloc(&e->d_n, 4));
  CREATE_TRY(dalloc(&e->d_total, 4));
  CREATE_TRY(dalloc(&e->d_stats, kStatBlk));
  e->d_sred = (unsigned long long*)(e->d_stats + kStatSred);
  e->d_inflight = e->d_stats + kStatInfl;
  CREATE_TRY(dalloc(&e->d_bstats, (uint64_t)kMaxApplyGrid * kBStats));
  CREATE_TRY(hipMemset(e->d_bstats, 0, (uint64_t)kMaxApplyGrid * kBStats * 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_heap_top, 2));
  CREATE_TRY(dalloc(&e->d_step, 1));
  CREATE_TRY(hipMemset(e->d_heap_top, 0, 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(hipMemset(e->d_step, 0, 4) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(dalloc(&e->d_cvec, AGX_MAX_RANKS + 2));
  CREATE_TRY(dalloc(&e->d_cmat, (uint64_t)AGX_MAX_RANKS * (AGX_MAX_RANKS + 2)));
  CREATE_TRY(hipMemset(e->d_n, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(hipMemset(e->d_total, 0, 16) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(hipMemset(e->d_stats, 0, kStatBlk * 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  CREATE_TRY(hipHostMalloc((void**)&e->h_stat, kStatBlk * 8, hipHostMallocDefault) == hipSuccess ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
  CREATE_TRY(hipHostMalloc((void**)&e->h_pin, 64 * 4, hipHostMallocDefault) == hipSuccess ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
  CREATE_TRY(hipHostMalloc((void**)&e->h_pin64, (AGX_MAX_RANKS * (AGX_MAX_RANKS + 2) + 8) * 8, hipHostMallocDefault) == hipSuccess ? AGX_OK : set_err(AGX_ENOMEM, "pinned"));
  // empty graph rows so FORWARD_RR on an engine without a graph is well defined
  e->h_row.assign(e->n_local + 1, 0);
  CREATE_TRY(dalloc(&e->d_row, e->n_local + 1));
  CREATE_TRY(hipMemset(e->d_row, 0, (e->n_local + 1) * 8) == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "memset"));
  // the hipMemsets above run on the null stream, which a non-blocking engine stream does not wait
  // for: without this, the first upload (prepare_run, on e->stream) could land before a memset of
  // the same buffer (seen: alive flags zeroed after their upload -> every tell a dead letter)
  CREATE_TRY(hipDeviceSynchronize() == hipSuccess ? AGX_OK : set_err(AGX_EDEVICE, "hipDeviceSynchronize"));
#undef CREATE_TRY
  *out = e;
  return AGX_OK;
}

agx_status agx_destroy(agx_engine* e) {
  if (!e) return AGX_OK;
  hipSetDevice((int)e->cfg.device);
  if (e->stream) hipStreamSynchronize(e->stream);
  // graphs first: a captured replay holds RCCL's persistent plans of this communicator, and
  // ncclCommDestroy with such a graph still alive never returned (round 5: the opt-in captured
  // multi-rank replay ran to quiescence, then the engine's destroy hung -- DESIGN.md §3.3)
  drop_graphs(e);
  const bool dbg = e->comm && getenv("AGX_MR_DEBUG");
  if (dbg) fprintf(stderr, "[agx rank %u] destroy: communicator\n", e->rank);
  if (e->comm) ncclCommDestroy(e->comm);
  if (dbg) fprintf(stderr, "[agx rank %u] destroy: communicator destroyed\n", e->rank);
  hipFree(e->d_kind); hipFree(e->d_alive); hipFree(e->d_stopq); hipFree(e->d_nstop); hipFree(e->d_state); hipFree(e->d_gid); hipFree(e->d_route);
  hipFree(e->d_zcdf); hipFree(e->d_zperm); hipFree(e->d_zent); hipFree(e->d_row); hipFree(e->d_col);
  free_msgs(e->A); free_msgs(e->B); free_msgs(e->scr); free_msgs(e->bl); free_msgs(e->em); free_msgs(e->stg);
  free_msgs(e->s2); free_msgs(e->bl2); free_msgs(e->eg0); free_msgs(e->eg1); free_msgs(e->em2);
  hipFree(e->d_emmeta); hipFree(e->d_slsum); hipFree(e->d_ident);
  hipFree(e->d_outbox); hipFree(e->d_outbox_n);
  hipFree(e->d_s2p); hipFree(e->d_rcvp); hipFree(e->d_sslab); hipFree(e->d_rslab); hipFree(e->d_halt);
  if (e->h_halt) hipHostFree(e->h_halt);
  for (int q = 0; q < 2; ++q) {
    hipFree(e->d_tcnt[q]); hipFree(e->d_toff[q]); hipFree(e->d_blo[q]); hipFree(e->d_blc[q]); hipFree(e->d_emc[q]);
  }
  hipFree(e->d_stg_off); hipFree(e->d_stg_cnt); hipFree(e->d_ovf); hipFree(e->d_cntb);
  if (e->h_cntb) hipHostFree(e->h_cntb); hipFree(e->d_parv);
  hipFree(e->d_abort); hipFree(e->d_rctr);
  hipFree(e->d_pbar);
  for (auto& ev : e->tev)
    if (ev) hipEventDestroy(ev);
  if (e->h_abort) hipHostFree(e->h_abort);
  hipFree(e->d_skew_list); hipFree(e->d_skew_n); hipFree(e->d_blist); hipFree(e->d_dense_left);
  hipFree(e->d_sk_rec); hipFree(e->d_sk_act); hipFree(e->d_sk_pc); hipFree(e->d_sk_meta);
  hipFree(e->d_ring_of); hipFree(e->d_ring_state); hipFree(e->d_ring_src); hipFree(e->d_ring_pay);
  hipFree(e->d_rg_state); hipFree(e->d_rg_nz); hipFree(e->d_rg_src); hipFree(e->d_rg_pay); hipFree(e->d_rg_dk); hipFree(e->d_rg_ds);
  hipFree(e->d_rg_dp);
  hipFree(e->d_ring_next); hipFree(e->d_ring_free); hipFree(e->d_ring_total);
  hipFree(e->d_orw); hipFree(e->d_orm); hipFree(e->d_orw_n); hipFree(e->d_lww_step0);
  hipFree(e->d_ptab);
  hipFree(e->d_stash);
  hipFree(e->d_timers);
  hipFree(e->d_watch);
  hipFree(e->d_child);
  hipFree(e->d_shard);
  hipFree(e->d_super);
  hipFree(e->d_backoff);
  hipFree(e->d_recep);
  hipFree(e->d_topic);
  hipFree(e->d_list);
  hipFree(e->d_hash);
  hipFree(e->d_chunk_off); hipFree(e->d_chunk_cnt); hipFree(e->d_hist_c); hipFree(e->d_hist_d); hipFree(e->d_tot); hipFree(e->d_bstart); hipFree(e->d_dbg);
  hipFree(e->d_moff0); hipFree(e->d_moff1); hipFree(e->d_blpre); hipFree(e->d_ninbox); hipFree(e->d_n); hipFree(e->d_total);
  hipFree(e->d_stats); hipFree(e->d_bstats); hipFree(e->d_cvec); hipFree(e->d_cmat);
  if (e->h_stat) hipHostFree(e->h_stat);
  for (auto ev : e->lag_ev)
    if (ev) hipEventDestroy(ev);
  hipFree(e->d_heap); hipFree(e->d_heap_top); hipFree(e->d_step); hipFree(e->d_rx); hipFree(e->d_s2rows); hipFree(e->d_srows);
  hipFree(e->d_bcase); hipFree(e->d_bact); hipFree(e->d_bfirst);
  if (e->h_pin) hipHostFree(e->h_pin);
  if (e->h_pin64) hipHostFree(e->h_pin64);
  for (auto ev : e->ev_pool) hipEventDestroy(ev);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
  return AGX_OK;
}

agx_status agx_register_range(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t kind, const void* init,
                              size_t stride) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));  // device state is authoritative after a run
  const bool compiled = kind >= AGX_KIND_COMPILED && kind < AGX_KIND_COMPILED + AGX_MAX_BEHAVIORS;
  const bool lww = kind == AGX_KIND_LWWMAP;
  const bool pnm = kind == AGX_KIND_PNCOUNTERMAP;
  const bool mmm = kind == AGX_KIND_ORMULTIMAP;
  if (first_id + count > e->n_global || (kind >= AGX_KIND_MAX && !compiled && !lww && !pnm && !mmm)) return set_err(AGX_EINVAL, "bad range or kind");
  if (mmm && e->R > 1) return set_err(AGX_EINVAL, "ORMultiMap replicas need a single-rank engine (n_ranks %u)", e->R);
  // an ORMultiMap engine holds ORMultiMap replicas only (unregistering, AGX_KIND_NONE, stays possible)
  if (count && kind != AGX_KIND_NONE && (mmm ? (e->kinds_mask & ~(kb(AGX_KIND_NONE) | kb(AGX_KIND_ORMULTIMAP))) != 0
                                             : (e->kinds_mask & kb(AGX_KIND_ORMULTIMAP)) != 0))
    return set_err(AGX_EINVAL, "ORMultiMap replicas and actors of another kind (%u) need separate engines", mmm ? 0u : kind);
  if (pnm && e->R > 1) return set_err(AGX_EINVAL, "PNCounterMap replicas need a single-rank engine (n_ranks %u)", e->R);
  // a PNCounterMap engine holds PNCounterMap replicas only (unregistering, AGX_KIND_NONE, stays possible)
  if (count && kind != AGX_KIND_NONE && (pnm ? (e->kinds_mask & ~(kb(AGX_KIND_NONE) | kb(AGX_KIND_PNCOUNTERMAP))) != 0
                                             : (e->kinds_mask & kb(AGX_KIND_PNCOUNTERMAP)) != 0))
    return set_err(AGX_EINVAL, "PNCounterMap replicas and actors of another kind (%u) need separate engines", pnm ? 0u : kind);
  if (lww && e->R > 1) return set_err(AGX_EINVAL, "LWWMap replicas need a single-rank engine (n_ranks %u)", e->R);
  // an LWWMap engine holds LWWMap replicas only (unregistering, AGX_KIND_NONE, stays possible)
  if (count && kind != AGX_KIND_NONE && (lww ? (e->kinds_mask & ~(kb(AGX_KIND_NONE) | kb(AGX_KIND_LWWMAP))) != 0
                                             : (e->kinds_mask & kb(AGX_KIND_LWWMAP)) != 0))
    return set_err(AGX_EINVAL, "LWWMap replicas and actors of another kind (%u) need separate engines", lww ? 0u : kind);
  const uint32_t kCrdtMask = kb(AGX_KIND_GCOUNTER) | kb(AGX_KIND_PNCOUNTER) | kb(AGX_KIND_ORSET);
  if (count && ((compiled && (e->kinds_mask & kCrdtMask)) ||
                (kind >= AGX_KIND_GCOUNTER && kind <= AGX_KIND_ORSET && (e->kinds_mask & kb(AGX_KIND_COMPILED)))))
    return set_err(AGX_EINVAL, "compiled behaviours and CRDT replicas need separate engines");
  if ((kind == AGX_KIND_FORWARD_RR || kind == AGX_KIND_STOP_AFTER) && e->W < 2)
    return set_err(AGX_EINVAL, "behaviour kind %u needs n_words >= 2", kind);
  if (init && stride < e->W * 8ull) return set_err(AGX_EINVAL, "state_stride smaller than n_words*8");
  for (const auto& r : e->ch_regions) {  // (children: the ids of a child block belong to the engine)
    const uint64_t c0 = r.first_child, c1 = c0 + (uint64_t)r.n_parents * r.max_children;
    if (count && first_id < c1 && c0 < first_id + count)
      return set_err(AGX_EINVAL, "register_range [%llu, %llu) overlaps the child block [%llu, %llu) (agx_set_children): "
                     "its actors are created by their parents", (unsigned long long)first_id,
                     (unsigned long long)(first_id + count), (unsigned long long)c0, (unsigned long long)c1);
  }
  for (const auto& t : e->sh_types) {  // (sharding: the ids of an entity range belong to the engine)
    const uint64_t c0 = t.first_id, c1 = c0 + t.count;
    if (count && first_id < c1 && c0 < first_id + count)
      return set_err(AGX_EINVAL, "register_range [%llu, %llu) overlaps the entity range [%llu, %llu) (agx_set_sharding): "
                     "its entities are started by their first message", (unsigned long long)first_id,
                     (unsigned long long)(first_id + count), (unsigned long long)c0, (unsigned long long)c1);
  }
  if ((kind >= AGX_KIND_GCOUNTER && kind <= AGX_KIND_ORSET) || lww || pnm || mmm) AGX_TRY(enable_crdt(e, kind));
  if (count && !(e->kinds_mask & kb(kind))) {  // the apply variant is captured in the superstep graphs
    e->kinds_mask |= kb(kind);
    drop_graphs(e);
  }
  const uint8_t* ib = (const uint8_t*)init;
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t id = first_id + i, l;
    if (e->R > 1) {
      uint32_t r = e->h_route[id];
      if ((r >> kOwnerShift) != e->rank) continue;
      l = r & kLocalMask;
    } else {
      l = id;
    }
    e->h_kind[l] = (uint8_t)kind;
    if (!e->h_init.empty()) e->h_init[l] = (uint8_t)kind;  // (supervision: the kind a restart returns to)
    e->h_alive[l] = (uint8_t)((e->h_alive[l] & 0xFEu) | (kind != AGX_KIND_NONE ? 1u : 0u));  // (bits 1..3: mailbox class)
    for (uint32_t w = 0; w < e->W; ++w) {
      uint64_t v = 0;
      if (ib) memcpy(&v, ib + i * stride + w * 8, 8);
      e->h_state[(uint64_t)w * e->n_local + l] = v;
    }
  }
  e->actors_dirty = true;
  return AGX_OK;
}

agx_status agx_set_mailbox_class(agx_engine* e, uint32_t cls, uint32_t capacity) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (cls == 0 || cls >= AGX_MAX_MAILBOX_CLASSES)
    return set_err(AGX_EINVAL, "mailbox class %u: classes 1..%u are configurable (0 is agx_cfg.capacity)", cls,
                   AGX_MAX_MAILBOX_CLASSES - 1);
  if (e->ring_live && (capacity == 0 || capacity > e->ring_c))
    return set_err(AGX_EINVAL,
                   "mailbox class %u capacity %u: this engine keeps queued messages in rings of %u (set every "
                   "mailbox class before the first run, or AGX_RING_SLOTS=0)", cls, capacity, e->ring_c);
  if (e->rg_on && (capacity == 0 || capacity > e->rg_c))
    return set_err(AGX_EINVAL,
                   "mailbox class %u capacity %u: this engine keeps queued messages in per-actor rings of %u (set "
                   "every mailbox class before the first run, or AGX_RING_APPLY=0)", cls, capacity, e->rg_c);
  e->mcap[cls] = capacity;
  e->mclass_set |= 1u << cls;
  e->mclasses = true;
  drop_graphs(e);  // the class table is a kernel parameter captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_set_mailbox(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t cls) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (cls >= AGX_MAX_MAILBOX_CLASSES || !((e->mclass_set >> cls) & 1u))
    return set_err(AGX_EINVAL, "mailbox class %u is not configured (agx_set_mailbox_class)", cls);
  if (first_id + count > e->n_global) return set_err(AGX_EINVAL, "bad actor range");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));  // device state is authoritative after a run
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t id = first_id + i;
    uint64_t l = id;
    if (e->R > 1) {
      const uint32_t r = e->h_route[id];
      if ((r >> kOwnerShift) != e->rank) continue;
      l = r & kLocalMask;
    }
    e->h_alive[l] = (uint8_t)((e->h_alive[l] & 1u) | (cls << 1));
  }
  e->actors_dirty = true;
  return AGX_OK;
}

// Mailbox.scala:726-816 (priority / stable priority), :867-1025 (control-aware)
agx_status agx_set_mailbox_priority(agx_engine* e, uint32_t cls, const uint8_t prio[256]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (cls >= AGX_MAX_MAILBOX_CLASSES || !((e->mclass_set >> cls) & 1u))
    return set_err(AGX_EINVAL, "mailbox class %u is not configured (agx_set_mailbox_class; classes 0..%u)", cls,
                   AGX_MAX_MAILBOX_CLASSES - 1);
  AGX_TRY(refuse_feature(e, F_PRIO));
  AGX_TRY(ensure_dev(e));
  if (prio) {
    memcpy(e->prio_tab.data() + cls * 256u, prio, 256);
    e->prio_mask |= 1u << cls;
  } else {
    memset(e->prio_tab.data() + cls * 256u, 0, 256);
    e->prio_mask &= ~(1u << cls);
  }
  e->prio_dirty = e->prio_mask != 0;
  drop_graphs(e);  // the variant and the tables are captured in the superstep graphs
  return AGX_OK;
}

// Stash.scala (classic `stash-capacity`, *DequeBasedMailbox); TY/internal/StashBufferImpl.scala:61-79,131-218
agx_status agx_set_stash(agx_engine* e, uint32_t cls, uint32_t capacity) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (cls >= AGX_MAX_MAILBOX_CLASSES || !((e->mclass_set >> cls) & 1u))
    return set_err(AGX_EINVAL, "mailbox class %u is not configured (agx_set_mailbox_class; classes 0..%u)", cls,
                   AGX_MAX_MAILBOX_CLASSES - 1);
  if (capacity == 0 || capacity > 255u)
    return set_err(AGX_EINVAL, "stash capacity %u: a stash holds 1..255 messages (there is no unbounded stash: "
                   "stash-capacity = -1 is not supported)", capacity);
  AGX_TRY(refuse_feature(e, F_STASH));
  AGX_TRY(ensure_dev(e));
  e->stash_cap[cls] = capacity;
  e->stash_on = true;
  e->stash_dirty = true;
  drop_graphs(e);  // the variant and the stash storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_stash_info(agx_engine* e, uint64_t* stashed, uint64_t* unstashed, uint64_t* overflows, uint64_t* held,
                          uint64_t* pending) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[3] = {0, 0, 0}, h = 0, p = 0, w = 0;
  if (e->d_stash) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, c, e->d_stash + kStashCtr, sizeof(c), hipMemcpyDeviceToHost));
    AGX_TRY(stash_scan(e, &h, &p, &w));
  }
  if (stashed) *stashed = c[0];
  if (unstashed) *unstashed = c[1];
  if (overflows) *overflows = c[2];
  if (held) *held = h;
  if (pending) *pending = p;
  return AGX_OK;
}

agx_status agx_read_stash(agx_engine* e, uint64_t actor_id, uint32_t* src, uint32_t* payload, uint32_t cap,
                          uint32_t* n_released, uint32_t* n) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  if (n) *n = 0;
  if (n_released) *n_released = 0;
  if (!e->d_stash) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  const uint64_t l = actor_id;  // (single rank: local = global)
  uint32_t h[2];
  AGX_TRY(copy_sync(e, h, e->d_stash + e->stash_hdr_off + 2ull * l, sizeof(h), hipMemcpyDeviceToHost));
  const uint32_t head = h[0] & 0xFFu, rel = (h[0] >> 8) & 0xFFu, size = (h[0] >> 16) & 0xFFu;
  if (n) *n = size;
  if (n_released) *n_released = rel;
  if (!size) return AGX_OK;
  const uint64_t per = (uint64_t)e->stash_smax + e->stash_pmax;
  std::vector<uint32_t> sl(2ull * e->stash_smax);
  AGX_TRY(copy_sync(e, sl.data(), e->d_stash + e->stash_slot_off + 2ull * l * per, sl.size() * 4ull, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < size && i < cap; ++i) {
    const uint32_t x = (head + i) % e->stash_smax;
    if (src) src[i] = sl[2 * x];
    if (payload) payload[i] = sl[2 * x + 1];
  }
  return AGX_OK;
}

// the behaviour kind of each actor now (a compiled behaviour's become and unstash_all change it)
agx_status agx_read_kinds(agx_engine* e, uint64_t first_id, uint64_t count, uint8_t* kinds) {
  if (!e || !kinds) return set_err(AGX_EINVAL, "null argument");
  if (e->R > 1) return set_err(AGX_EINVAL, "agx_read_kinds needs a single-rank engine");
  if (first_id + count > e->n_global) return set_err(AGX_EINVAL, "bad actor range");
  AGX_TRY(ensure_dev(e));
  if (e->actors_dirty) {  // the host mirror is newer than the device
    memcpy(kinds, e->h_kind.data() + first_id, count);
    return AGX_OK;
  }
  if (count) AGX_TRY(copy_sync(e, kinds, e->d_kind + first_id, count, hipMemcpyDeviceToHost));
  return AGX_OK;
}

// TY/internal/TimerSchedulerImpl.scala:61-172 (classic dungeon/TimerSchedulerImpl.scala: the same rule)
agx_status agx_set_timers(agx_engine* e, uint32_t n_keys) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (n_keys < 1u || n_keys > AGX_MAX_TIMER_KEYS)
    return set_err(AGX_EINVAL, "timers: %u keys per actor (1..%u)", n_keys, AGX_MAX_TIMER_KEYS);
  AGX_TRY(refuse_feature(e, F_TIMERS));
  if (e->rt_on && n_keys != e->tm_keys)
    return set_err(AGX_EINVAL, "timers: the key count cannot change once receive timeouts are set (agx_set_receive_timeout)");
  if (e->ask_on && n_keys != e->tm_keys)
    return set_err(AGX_EINVAL, "timers: the key count cannot change once the ask pattern is set (agx_set_ask)");
  AGX_TRY(ensure_dev(e));
  if (e->d_timers && n_keys != e->tm_keys) {
    hipFree(e->d_timers);
    e->d_timers = nullptr;
    e->tm_starts.clear();
  }
  e->tm_keys = n_keys;
  e->tm_bad_start = false;  // (an agx_start_timers refused before this call no longer stands in the way of agx_run)
  AGX_TRY(alloc_timers(e));  // (now: AGX_ENOMEM is this call's)
  drop_graphs(e);  // the variant and the timer storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_start_timers(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t key, int32_t periodic, uint32_t delay,
                            const uint32_t* delays, uint32_t payload) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->tm_keys) {
    e->tm_bad_start = true;  // (agx_run refuses too: the rule for tables with timer actions)
    return set_err(AGX_EINVAL, "agx_start_timers needs an engine with timers (agx_set_timers)");
  }
  if (key >= e->tm_keys) return set_err(AGX_EINVAL, "timer key %u: the engine has %u slots per actor", key, e->tm_keys);
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  if (e->rt_on && (payload >> 24) == AGX_TAG_RECEIVE_TIMEOUT)
    return set_err(AGX_EINVAL, "agx_start_timers: message tag 0xFB is reserved for receive-timeout envelopes on an engine "
                   "with receive timeouts");
  agx_engine::TimerStart ts;
  ts.first = first_id;
  ts.count = count;
  ts.key = key;
  ts.periodic = periodic ? 1u : 0u;
  ts.delay = delay;
  ts.payload = payload;
  if (delays) ts.delays.assign(delays, delays + count);
  e->tm_starts.push_back(std::move(ts));
  return AGX_OK;
}

agx_status agx_timer_info(agx_engine* e, uint64_t* fired, uint64_t* discarded, uint64_t* active, uint64_t* pending,
                          uint64_t* ticks) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[2] = {0, 0}, na = 0, npd = 0;
  if (e->d_timers) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_timer_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
    AGX_TRY(copy_sync(e, c, e->d_timers + kTmCtr, sizeof(c), hipMemcpyDeviceToHost));
    const uint64_t npad = (uint64_t)e->nb << e->bb;
    std::vector<uint32_t> sl(2ull * e->tm_keys * npad);  // next, per
    AGX_TRY(copy_sync(e, sl.data(), e->d_timers + tm_slot_off(e->nb), sl.size() * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < e->tm_keys; ++k)
      for (uint64_t l = 0; l < e->n_local; ++l) {
        if (!(sl[((uint64_t)e->tm_keys + k) * npad + l] & kTmActive)) continue;
        ++na;
        npd += sl[k * npad + l] != kTmNone;
      }
  }
  if (fired) *fired = c[0];
  if (discarded) *discarded = c[1];
  if (active) *active = na;
  if (pending) *pending = npd;
  if (ticks) *ticks = e->tm_ticks;
  return AGX_OK;
}

agx_status agx_read_timers(agx_engine* e, uint64_t actor_id, uint32_t active[4], uint32_t remaining[4], uint32_t period[4],
                           uint32_t payload[4], uint32_t generation[4]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  for (uint32_t k = 0; k < AGX_MAX_TIMER_KEYS; ++k) {
    if (active) active[k] = 0;
    if (remaining) remaining[k] = 0xFFFFFFFFu;
    if (period) period[k] = 0;
    if (payload) payload[k] = 0;
    if (generation) generation[k] = 0;
  }
  if (!e->d_timers) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_timer_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
  const uint64_t npad = (uint64_t)e->nb << e->bb, l = actor_id;  // (single rank: local = global)
  uint32_t clk = 0;
  AGX_TRY(copy_sync(e, &clk, e->d_timers + kTmBucketOff + 2ull * e->nb + (l >> e->bb), 4, hipMemcpyDeviceToHost));
  // the actor's column of the [field][key][actor] arrays in one strided copy: row f * n_keys + k = field f of key k
  uint32_t col[4 * AGX_MAX_TIMER_KEYS];
  HIP_TRY(hipMemcpy2DAsync(col, 4, e->d_timers + tm_slot_off(e->nb) + l, npad * 4ull, 4, 4ull * e->tm_keys,
                           hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (uint32_t k = 0; k < e->tm_keys; ++k) {
    const uint32_t v[4] = {col[k], col[e->tm_keys + k], col[2 * e->tm_keys + k], col[3 * e->tm_keys + k]};
    if (active) active[k] = (v[1] & kTmActive) ? 1u : 0u;
    if (remaining) remaining[k] = v[0] == kTmNone ? 0xFFFFFFFFu : v[0] - clk;
    if (period) period[k] = v[1] & ~kTmActive;
    if (payload) payload[k] = v[3];
    if (generation) generation[k] = v[2];
  }
  return AGX_OK;
}

// AA/dungeon/ReceiveTimeout.scala:18-74 (typed: TY/internal/adapter/ActorContextAdapter.scala:120-131)
agx_status agx_set_receive_timeout(agx_engine* e, const uint32_t transparent_tags[8]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->tm_keys) return set_err(AGX_EINVAL, "receive timeouts need an engine with timers (agx_set_timers first)");
  if (e->started) return set_err(AGX_ESTATE, "set receive timeouts before the first agx_run");
  if (e->rt_on) return set_err(AGX_EINVAL, "receive timeouts are set already (agx_set_receive_timeout is called once)");
  if (e->ask_on)
    return set_err(AGX_EINVAL, "receive timeouts need an engine without the ask pattern (agx_set_ask): the two are features of "
                   "their own on top of the timers");
  if (e->beh_rt_tag)
    return set_err(AGX_EINVAL, "receive timeouts: the compiled behaviours name message tag 0xFB, reserved for receive-timeout "
                   "envelopes");
  for (const auto& ts : e->tm_starts)
    if ((ts.payload >> 24) == AGX_TAG_RECEIVE_TIMEOUT)
      return set_err(AGX_EINVAL, "receive timeouts: a recorded agx_start_timers payload carries message tag 0xFB, reserved for "
                     "receive-timeout envelopes");
  if (e->hs_pay.end() != std::find_if(e->hs_pay.begin(), e->hs_pay.end(),
                                      [](uint32_t p) { return (p >> 24) == AGX_TAG_RECEIVE_TIMEOUT; }))
    return set_err(AGX_EINVAL, "receive timeouts: a staged tell carries message tag 0xFB, reserved for receive-timeout "
                   "envelopes");
  AGX_TRY(ensure_dev(e));
  for (uint32_t i = 0; i < 8; ++i) e->rt_mask[i] = transparent_tags ? transparent_tags[i] : 0u;
  // the storage grows by the three rows and the mask: allocated anew (no timer has run; recorded starts are kept)
  hipFree(e->d_timers);
  e->d_timers = nullptr;
  e->rt_on = true;
  e->rt_bad_start = false;  // (an agx_start_receive_timeout refused before this call no longer stands in the way of agx_run)
  const agx_status r = alloc_timers(e);  // (now: AGX_ENOMEM is this call's)
  if (r != AGX_OK) {
    e->rt_on = false;
    (void)alloc_timers(e);
    return r;
  }
  drop_graphs(e);  // the variant and the timer storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_start_receive_timeout(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t delay, uint32_t payload) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->rt_on) {
    e->rt_bad_start = true;  // (agx_run refuses too: the rule for tables that set a receive timeout)
    return set_err(AGX_EINVAL, "agx_start_receive_timeout needs an engine with receive timeouts (agx_set_receive_timeout)");
  }
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  if (delay && (payload >> 24) == AGX_TAG_RECEIVE_TIMEOUT)
    return set_err(AGX_EINVAL, "agx_start_receive_timeout: message tag 0xFB is reserved for receive-timeout envelopes");
  e->rt_starts.push_back({first_id, count, delay, payload});
  return AGX_OK;
}

agx_status agx_receive_timeout_info(agx_engine* e, uint64_t* fired, uint64_t* discarded, uint64_t* set, uint64_t* pending) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[2] = {0, 0}, ns = 0, npd = 0;
  if (e->rt_on && e->d_timers) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_timer_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
    AGX_TRY(copy_sync(e, c, e->d_timers + kRtCtr, sizeof(c), hipMemcpyDeviceToHost));
    const uint64_t npad = (uint64_t)e->nb << e->bb;
    std::vector<uint32_t> rows(2ull * npad);  // rt_next, rt_delay
    AGX_TRY(copy_sync(e, rows.data(), e->d_timers + rt_row_off(e), rows.size() * 4ull, hipMemcpyDeviceToHost));
    for (uint64_t l = 0; l < e->n_local; ++l) {
      if (!rows[npad + l]) continue;
      ++ns;
      npd += rows[l] != kTmNone;
    }
  }
  if (fired) *fired = c[0];
  if (discarded) *discarded = c[1];
  if (set) *set = ns;
  if (pending) *pending = npd;
  return AGX_OK;
}

agx_status agx_read_receive_timeout(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t* delay, uint32_t* remaining,
                                    uint32_t* payload) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  for (uint64_t i = 0; i < count; ++i) {
    if (delay) delay[i] = 0;
    if (remaining) remaining[i] = 0xFFFFFFFFu;
    if (payload) payload[i] = 0;
  }
  if (!e->rt_on || !e->d_timers || !count) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_timer_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  uint32_t clk = 0;  // (every bucket's clock holds the tick count)
  AGX_TRY(copy_sync(e, &clk, e->d_timers + kTmBucketOff + 2ull * e->nb, 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> nx(count);
  AGX_TRY(copy_sync(e, nx.data(), e->d_timers + rt_row_off(e) + first_id, count * 4ull, hipMemcpyDeviceToHost));
  if (delay) AGX_TRY(copy_sync(e, delay, e->d_timers + rt_row_off(e) + npad + first_id, count * 4ull, hipMemcpyDeviceToHost));
  if (payload) AGX_TRY(copy_sync(e, payload, e->d_timers + rt_row_off(e) + 2ull * npad + first_id, count * 4ull, hipMemcpyDeviceToHost));
  if (remaining)
    for (uint64_t i = 0; i < count; ++i) remaining[i] = nx[i] == kTmNone ? 0xFFFFFFFFu : nx[i] - clk;
  return AGX_OK;
}

// akka-cluster-sharding Shard.scala:388-516
agx_status agx_set_sharding(agx_engine* e, const agx_entity_type* types, uint32_t n_types) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->rt_on)
    return set_err(AGX_EINVAL, "sharding needs an engine with receive timeouts (agx_set_timers, then agx_set_receive_timeout "
                   "first)");
  if (e->started) return set_err(AGX_ESTATE, "set sharding before the first agx_run");
  if (e->d_shard) return set_err(AGX_EINVAL, "sharding is set already (agx_set_sharding is called once)");
  if (n_types < 1u || n_types > AGX_MAX_ENTITY_TYPES || !types)
    return set_err(AGX_EINVAL, "sharding: %u entity types (1..%u)", n_types, AGX_MAX_ENTITY_TYPES);
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));
  const uint64_t n = e->n_global;
  for (uint32_t i = 0; i < n_types; ++i) {
    const agx_entity_type& t = types[i];
    const uint64_t c0 = t.first_id, c1 = c0 + t.count;
    if (!t.count || c1 > n) return set_err(AGX_EINVAL, "sharding: entity type %u is empty or leaves [0, n_actors)", i);
    for (uint32_t j = 0; j < i; ++j) {
      const uint64_t d0 = types[j].first_id, d1 = d0 + types[j].count;
      if (c0 < d1 && d0 < c1) return set_err(AGX_EINVAL, "sharding: the ranges of entity types %u and %u overlap", j, i);
    }
    if (t.kind < AGX_KIND_COMPILED || t.kind >= AGX_KIND_COMPILED + AGX_MAX_BEHAVIORS || (t.flags & ~AGX_ENTITY_WORD1_ID) ||
        t.reserved)
      return set_err(AGX_EINVAL, "sharding: entity type %u: kind %u is no compiled behaviour kind, or unknown flags", i, t.kind);
    const uint32_t st = t.stop_payload >> 24, it = t.idle_payload >> 24;
    if (st == AGX_TAG_TIMER || st == AGX_TAG_RECEIVE_TIMEOUT || (t.idle_delay && (it == AGX_TAG_TIMER || it == AGX_TAG_RECEIVE_TIMEOUT)))
      return set_err(AGX_EINVAL, "sharding: entity type %u: a stop or idle message carries a reserved tag (0xFF, 0xFB)", i);
    for (uint64_t x = c0; x < c1; ++x)
      if (e->h_alive[x] & 1u)
        return set_err(AGX_EINVAL, "sharding: id %llu of entity type %u's range is registered", (unsigned long long)x, i);
  }
  AGX_TRY(alloc_timers(e));
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  const size_t total = kShRowOff + 3ull * npad;
  if (hipMalloc((void**)&e->d_shard, total * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_shard = nullptr;
    return set_err(AGX_ENOMEM, "the entity storage of %llu actors does not fit on the device", (unsigned long long)n);
  }
  std::vector<uint32_t> h(kShRowOff, 0u);
  h[0] = n_types;
  for (uint32_t i = 0; i < n_types; ++i) {
    uint32_t* T = &h[kShTypeOff + kShTypeWords * i];
    T[0] = types[i].first_id;
    T[1] = types[i].count;
    T[2] = types[i].kind;
    T[3] = types[i].flags;
    T[4] = (uint32_t)types[i].base0;
    T[5] = (uint32_t)(types[i].base0 >> 32);
    T[6] = (uint32_t)types[i].word1;
    T[7] = (uint32_t)(types[i].word1 >> 32);
    T[8] = types[i].stop_payload;
    T[9] = std::min(types[i].idle_delay, kTmMaxDelay);
    T[10] = types[i].idle_payload;
  }
  HIP_TRY(hipMemsetAsync(e->d_shard, 0, total * 4ull, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_shard, h.data(), h.size() * 4ull, hipMemcpyHostToDevice, e->stream));
  const unsigned long long addr = (unsigned long long)(uintptr_t)e->d_shard;
  HIP_TRY(hipMemcpyAsync(e->d_timers + kTmShardPtr, &addr, 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->sh_types.assign(types, types + n_types);
  if (!(e->kinds_mask & kb(AGX_KIND_COMPILED))) e->kinds_mask |= kb(AGX_KIND_COMPILED);  // (the entities' kinds)
  drop_graphs(e);  // the variant is captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_sharding_info(agx_engine* e, uint64_t* started, uint64_t* restarted, uint64_t* passivations, uint64_t* passivated,
                             uint64_t* passivate_ignored, uint64_t* passivate_unknown, uint64_t* alive) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[kScN] = {0, 0, 0, 0, 0, 0}, na = 0;
  if (e->d_shard) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, c, e->d_shard + kShCtr, sizeof(c), hipMemcpyDeviceToHost));
    AGX_TRY(sync_mirrors(e));  // (the flags of the device are the newer ones after a run)
    for (const auto& t : e->sh_types)
      for (uint64_t x = t.first_id; x < (uint64_t)t.first_id + t.count; ++x) na += e->h_alive[x] & 1u;
  }
  if (started) *started = c[kScStarted];
  if (restarted) *restarted = c[kScRestarted];
  if (passivations) *passivations = c[kScPassivations];
  if (passivated) *passivated = c[kScPassivated];
  if (passivate_ignored) *passivate_ignored = c[kScIgnored];
  if (passivate_unknown) *passivate_unknown = c[kScUnknown];
  if (alive) *alive = na;
  return AGX_OK;
}

agx_status agx_read_entities(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t* alive, uint32_t* incarnations,
                             uint32_t* passivating) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));
  std::vector<uint32_t> st(count, 0u);
  if (e->d_shard && count) AGX_TRY(copy_sync(e, st.data(), e->d_shard + kShRowOff + first_id, count * 4ull, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < count; ++i) {
    if (alive) alive[i] = e->h_alive[first_id + i] & 1u;
    if (incarnations) incarnations[i] = st[i] & ~kShPassivating;
    if (passivating) passivating[i] = (st[i] & kShPassivating) ? 1u : 0u;
  }
  return AGX_OK;
}

// TY/internal/ActorContextImpl.scala:203-218, TY/scaladsl/AskPattern.scala:109-162
agx_status agx_set_ask(agx_engine* e) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->tm_keys) return set_err(AGX_EINVAL, "the ask pattern needs an engine with timers (agx_set_timers first)");
  if (e->started) return set_err(AGX_ESTATE, "set the ask pattern before the first agx_run");
  if (e->ask_on) return set_err(AGX_EINVAL, "the ask pattern is set already (agx_set_ask is called once)");
  if (e->rt_on)
    return set_err(AGX_EINVAL, "the ask pattern needs an engine without receive timeouts (agx_set_receive_timeout): the two are "
                   "features of their own on top of the timers");
  if (e->n_global > AGX_ASK_MAX_ACTORS)
    return set_err(AGX_EINVAL, "the ask pattern needs an engine of at most %u actors (it has %llu): an ask ref carries the "
                   "asker's id in 22 bits", AGX_ASK_MAX_ACTORS, (unsigned long long)e->n_global);
  AGX_TRY(ensure_dev(e));
  // the storage grows by the ask row: allocated anew (no timer has run; recorded starts are kept)
  hipFree(e->d_timers);
  e->d_timers = nullptr;
  e->ask_on = true;
  const agx_status r = alloc_timers(e);  // (now: AGX_ENOMEM is this call's)
  if (r != AGX_OK) {
    e->ask_on = false;
    (void)alloc_timers(e);
    return r;
  }
  drop_graphs(e);  // the variant and the timer storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_ask_info(agx_engine* e, uint64_t* asked, uint64_t* answered, uint64_t* timed_out, uint64_t* late) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[kAcN] = {0, 0, 0, 0};
  if (e->ask_on && e->d_timers) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, c, e->d_timers + kAskCtr, sizeof(c), hipMemcpyDeviceToHost));
  }
  if (asked) *asked = c[kAcAsked];
  if (answered) *answered = c[kAcAnswered];
  if (timed_out) *timed_out = c[kAcTimedOut];
  if (late) *late = c[kAcLate];
  return AGX_OK;
}

agx_status agx_read_asks(agx_engine* e, uint64_t actor_id, uint32_t is_ask[4], uint32_t adapt[4]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  for (uint32_t k = 0; k < AGX_MAX_TIMER_KEYS; ++k) {
    if (is_ask) is_ask[k] = 0;
    if (adapt) adapt[k] = 0xFFFFFFFFu;
  }
  if (!e->ask_on || !e->d_timers) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_timer_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
  const uint64_t npad = (uint64_t)e->nb << e->bb, l = actor_id;  // (single rank: local = global)
  uint32_t per[AGX_MAX_TIMER_KEYS], row[AGX_MAX_TIMER_KEYS];  // the actor's column of per[key][actor] and ask[key][actor]
  HIP_TRY(hipMemcpy2DAsync(per, 4, e->d_timers + tm_slot_off(e->nb) + (uint64_t)e->tm_keys * npad + l, npad * 4ull, 4, e->tm_keys,
                           hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpy2DAsync(row, 4, e->d_timers + ask_row_off(e) + l, npad * 4ull, 4, e->tm_keys, hipMemcpyDeviceToHost,
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (uint32_t k = 0; k < e->tm_keys; ++k) {
    const bool on = (per[k] & kTmActive) && (row[k] & kAskIs);
    if (is_ask) is_ask[k] = on ? 1u : 0u;
    if (adapt) adapt[k] = on && (row[k] & kAskHasTag) ? row[k] & 0xFFu : 0xFFFFFFFFu;
  }
  return AGX_OK;
}

// AA/dungeon/DeathWatch.scala:19-113 (typed adapter: TY/internal/adapter/ActorAdapter.scala:84-91,134-138,200-205)
agx_status agx_set_death_watch(agx_engine* e, uint32_t n_slots) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (n_slots < 1u || n_slots > AGX_MAX_WATCH_SLOTS)
    return set_err(AGX_EINVAL, "death watch: %u slots per actor (1..%u)", n_slots, AGX_MAX_WATCH_SLOTS);
  AGX_TRY(refuse_feature(e, F_WATCH));
  AGX_TRY(ensure_dev(e));
  if (e->d_child && n_slots != e->wd_slots)
    return set_err(AGX_EINVAL, "death watch: the slot count cannot change once children are set (agx_set_children)");
  if (e->d_watch && n_slots != e->wd_slots) {
    hipFree(e->d_watch);
    e->d_watch = nullptr;
    e->wd_starts.clear();
  }
  e->wd_slots = n_slots;
  e->wd_bad_start = false;  // (an agx_start_watch refused before this call no longer stands in the way of agx_run)
  AGX_TRY(alloc_watch(e));  // (now: AGX_ENOMEM is this call's)
  drop_graphs(e);  // the variant and the watch storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_start_watch(agx_engine* e, uint64_t first_id, uint64_t count, const uint32_t* watchees, int64_t offset,
                           int32_t with_message, uint32_t payload) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->wd_slots) {
    e->wd_bad_start = true;  // (agx_run refuses too: the rule for tables with watch actions)
    return set_err(AGX_EINVAL, "agx_start_watch needs an engine with death watch (agx_set_death_watch)");
  }
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  agx_engine::WatchStart ws;
  ws.first = first_id;
  ws.count = count;
  ws.offset = offset;
  ws.with = with_message ? 1u : 0u;
  ws.payload = payload;
  if (watchees) ws.watchees.assign(watchees, watchees + count);
  e->wd_starts.push_back(std::move(ws));
  return AGX_OK;
}

agx_status agx_watch_info(agx_engine* e, uint64_t* watches, uint64_t* terminated, uint64_t* discarded, uint64_t* death_pacts,
                          uint64_t* conflicts, uint64_t* watching, uint64_t* pending, uint64_t* ticks) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[5] = {0, 0, 0, 0, 0}, nw = 0, npd = 0;
  if (e->d_watch) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_watch_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
    AGX_TRY(copy_sync(e, c, e->d_watch + kWdCtr, sizeof(c), hipMemcpyDeviceToHost));
    const uint64_t npad = (uint64_t)e->nb << e->bb;
    std::vector<uint32_t> st((uint64_t)e->wd_slots * npad);
    AGX_TRY(copy_sync(e, st.data(), e->d_watch + wd_slot_off(e->nb) + (uint64_t)e->wd_slots * npad, st.size() * 4ull,
                      hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < e->wd_slots; ++k)
      for (uint64_t l = 0; l < e->n_local; ++l) {
        const uint32_t s = st[k * npad + l] & kWdStateMask;
        nw += s == kWdWatching;
        npd += s == kWdDue;
      }
  }
  if (watches) *watches = c[kWcWatches];
  if (terminated) *terminated = c[kWcTerminated];
  if (discarded) *discarded = c[kWcDiscarded];
  if (death_pacts) *death_pacts = c[kWcPacts];
  if (conflicts) *conflicts = c[kWcConflicts];
  if (watching) *watching = nw;
  if (pending) *pending = npd;
  if (ticks) *ticks = e->wd_ticks;
  return AGX_OK;
}

agx_status agx_read_watch(agx_engine* e, uint64_t actor_id, uint32_t watchee[4], uint32_t state[4], uint32_t payload[4],
                          uint32_t generation[4]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  for (uint32_t k = 0; k < AGX_MAX_WATCH_SLOTS; ++k) {
    if (watchee) watchee[k] = 0;
    if (state) state[k] = 0;
    if (payload) payload[k] = 0;
    if (generation) generation[k] = 0;
  }
  if (!e->d_watch) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_watch_starts(e));  // (starts recorded since the last run: applied now, nothing else is uploaded)
  const uint64_t npad = (uint64_t)e->nb << e->bb, l = actor_id;  // (single rank: local = global)
  // the actor's column of the [field][slot][actor] arrays in one strided copy: row f * n_slots + k = field f of slot k
  uint32_t col[4 * AGX_MAX_WATCH_SLOTS];
  HIP_TRY(hipMemcpy2DAsync(col, 4, e->d_watch + wd_slot_off(e->nb) + l, npad * 4ull, 4, 4ull * e->wd_slots,
                           hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (uint32_t k = 0; k < e->wd_slots; ++k) {
    if (watchee) watchee[k] = col[k];
    if (state) state[k] = col[e->wd_slots + k];
    if (generation) generation[k] = col[2 * e->wd_slots + k];
    if (payload) payload[k] = col[3 * e->wd_slots + k];
  }
  return AGX_OK;
}

// TY/internal/Supervision.scala:43-52,128-160,311-406
agx_status agx_set_supervision(agx_engine* e, const agx_supervisor* table, uint32_t n_behaviors, uint32_t n_levels) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!table || n_levels < 1u || n_levels > AGX_MAX_SUPERVISORS || n_behaviors < 1u || n_behaviors > AGX_MAX_BEHAVIORS)
    return set_err(AGX_EINVAL, "supervision: %u levels (1..%u) for %u behaviours (1..%u)", n_levels, AGX_MAX_SUPERVISORS,
                   n_behaviors, AGX_MAX_BEHAVIORS);
  for (uint32_t i = 0; i < n_behaviors * n_levels; ++i) {
    const agx_supervisor& S = table[i];
    if (!S.class_mask) continue;  // (an unused entry)
    if (S.strategy < AGX_SUP_RESUME || S.strategy > AGX_SUP_STOP || S.reset_mask > 3u ||
        (S.strategy == AGX_SUP_RESTART && (S.max_restarts < -1 || S.within < 1u)))
      return set_err(AGX_EINVAL, "supervision: bad entry %u of behaviour %u (a strategy, reset words 0..1, max_restarts >= -1, "
                     "within >= 1 tick)", i % n_levels, i / n_levels);
  }
  AGX_TRY(refuse_feature(e, F_SUPER));
  AGX_TRY(ensure_dev(e));
  if (e->d_super && n_levels != e->sv_levels) {
    hipFree(e->d_super);
    e->d_super = nullptr;
  }
  e->sv_on = true;
  e->sv_levels = n_levels;
  e->sv_beh = n_behaviors;
  e->sv_tab.assign((size_t)AGX_MAX_BEHAVIORS * AGX_MAX_SUPERVISORS, agx_supervisor{});
  for (uint32_t b = 0; b < n_behaviors; ++b)
    for (uint32_t k = 0; k < n_levels; ++k) e->sv_tab[(size_t)b * AGX_MAX_SUPERVISORS + k] = table[(size_t)b * n_levels + k];
  e->h_init = e->h_kind;  // (before the first run the mirror holds the kinds the actors were registered with)
  e->sv_init_dirty = true;
  AGX_TRY(alloc_super(e));  // (now: AGX_ENOMEM is this call's)
  drop_graphs(e);  // the variant and the supervision storage are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_supervision_info(agx_engine* e, uint64_t* failures, uint64_t* resumes, uint64_t* restarts, uint64_t* stops,
                                uint64_t* ticks) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[4] = {0, 0, 0, 0};
  if (e->d_super) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, c, e->d_super + kSvCtr, sizeof(c), hipMemcpyDeviceToHost));
  }
  if (failures) *failures = c[kScFailures];
  if (resumes) *resumes = c[kScResumes];
  if (restarts) *restarts = c[kScRestarts];
  if (stops) *stops = c[kScStops];
  if (ticks) *ticks = e->sv_ticks;
  return AGX_OK;
}

agx_status agx_read_supervision(agx_engine* e, uint64_t actor_id, uint32_t* initial_kind, uint32_t count[4],
                                uint32_t remaining[4]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  for (uint32_t k = 0; k < AGX_MAX_SUPERVISORS; ++k) {
    if (count) count[k] = 0;
    if (remaining) remaining[k] = 0xFFFFFFFFu;
  }
  if (initial_kind) *initial_kind = e->h_init.empty() ? 0u : e->h_init[actor_id];  // (single rank: local = global)
  if (!e->d_super) return AGX_OK;
  AGX_TRY(ensure_dev(e));
  const uint64_t npad = (uint64_t)e->nb << e->bb, l = actor_id;
  // the actor's column of count[level][actor], deadline[level][actor] in one strided copy
  uint32_t col[2 * AGX_MAX_SUPERVISORS];
  HIP_TRY(hipMemcpy2DAsync(col, 4, e->d_super + sv_ent_off(e->nb) + kSvEntWords + l, npad * 4ull, 4, 2ull * e->sv_levels,
                           hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (uint32_t k = 0; k < e->sv_levels; ++k) {
    const uint32_t d = col[e->sv_levels + k];
    if (count) count[k] = col[k];
    if (remaining) remaining[k] = d == 0u ? 0xFFFFFFFFu : (uint64_t)d > e->sv_ticks ? (uint32_t)(d - e->sv_ticks) : 0u;
  }
  return AGX_OK;
}

// TY/internal/Supervision.scala:163-406
agx_status agx_set_backoff(agx_engine* e, const agx_backoff* table, uint32_t n_behaviors, uint32_t n_levels) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->sv_on) return set_err(AGX_EINVAL, "backoff needs an engine with supervision (agx_set_supervision first)");
  if (e->d_backoff) return set_err(AGX_EINVAL, "backoff is set once (agx_set_supervision with another table drops the rows)");
  if (!table || n_behaviors != e->sv_beh || n_levels != e->sv_levels)
    return set_err(AGX_EINVAL, "backoff: %u levels for %u behaviours; agx_set_supervision had %u levels for %u behaviours",
                   n_levels, n_behaviors, e->sv_levels, e->sv_beh);
  for (uint32_t i = 0; i < n_behaviors * n_levels; ++i) {
    const agx_backoff& R = table[i];
    if (!R.min_backoff) continue;  // (the entry stays a plain restart)
    if (R.min_backoff > R.max_backoff || R.max_backoff > 0x7FFFFFFFu || R.random_factor_q16 > 65536u || R.reset_after < 1u ||
        R.stash_capacity < -1)
      return set_err(AGX_EINVAL, "backoff: bad row %u of behaviour %u (1 <= min_backoff <= max_backoff <= 2^31 - 1 ticks, "
                     "random_factor_q16 <= 65536, reset_after >= 1 tick, stash_capacity >= -1)", i % n_levels, i / n_levels);
    const agx_supervisor& S = e->sv_tab[(size_t)(i / n_levels) * AGX_MAX_SUPERVISORS + i % n_levels];
    if (!S.class_mask || S.strategy != AGX_SUP_RESTART)
      return set_err(AGX_EINVAL, "backoff: row %u of behaviour %u stands on an entry that is not AGX_SUP_RESTART", i % n_levels,
                     i / n_levels);
  }
  if (e->started) return set_err(AGX_ESTATE, "set backoff before the first agx_run");
  AGX_TRY(ensure_dev(e));
  e->bo_tab.assign((size_t)AGX_MAX_BEHAVIORS * AGX_MAX_SUPERVISORS, agx_backoff{});
  for (uint32_t b = 0; b < n_behaviors; ++b)
    for (uint32_t k = 0; k < n_levels; ++k) e->bo_tab[(size_t)b * AGX_MAX_SUPERVISORS + k] = table[(size_t)b * n_levels + k];
  const uint64_t npad = (uint64_t)e->nb << e->bb;
  const size_t total = bo_until_off(e->nb) + 3ull * npad;
  // (the engine names the storage only when it is whole and the SuperDev header points to it: a call that fails on the
  // way leaves an engine without backoff, which launches the supervision instantiation)
  uint32_t* d = nullptr;
  if (hipMalloc((void**)&d, total * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->bo_tab.clear();
    return set_err(AGX_ENOMEM, "the backoff state of %llu actors (%llu MB) does not fit on the device",
                   (unsigned long long)npad, (unsigned long long)(total >> 18));
  }
  std::vector<uint32_t> rows((size_t)AGX_MAX_BEHAVIORS * AGX_MAX_SUPERVISORS * kBoRowWords, 0u);
  for (size_t i = 0; i < e->bo_tab.size(); ++i) memcpy(&rows[i * kBoRowWords], &e->bo_tab[i], sizeof(agx_backoff));
  const uint64_t addr = (uint64_t)(uintptr_t)d;
  hipError_t he = hipMemsetAsync(d, 0, total * 4ull, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(d, &e->sv_levels, 4, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(d + bo_row_off(e->nb), rows.data(), rows.size() * 4ull, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_super + kSvBackoff, &addr, 8, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  if (he != hipSuccess) {
    hipFree(d);
    e->bo_tab.clear();
    HIP_TRY(he);
  }
  e->d_backoff = d;
  e->bo_sv = e->sv_tab;
  e->bo_levels = e->sv_levels;
  e->bo_beh = e->sv_beh;
  drop_graphs(e);  // the instantiation is captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_backoff_info(agx_engine* e, uint64_t* backoffs, uint64_t* resumed, uint64_t* dropped, uint64_t* limit_stops,
                            uint64_t* suspended) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[3] = {0, 0, 0}, susp = 0;
  if (e->d_backoff) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, c, e->d_backoff + kBoCtr, sizeof(c), hipMemcpyDeviceToHost));
    // suspended now: the actors that will not drain in the next tick (until > ticks + 1); `resumed` is derived
    std::vector<uint32_t> until(e->n_local);
    AGX_TRY(copy_sync(e, until.data(), e->d_backoff + bo_until_off(e->nb), (size_t)e->n_local * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t u : until) susp += (uint64_t)u > e->sv_ticks + 1ull ? 1u : 0u;
  }
  if (backoffs) *backoffs = c[kBcBackoffs];
  if (resumed) *resumed = c[kBcBackoffs] - susp;
  if (dropped) *dropped = c[kBcDropped];
  if (limit_stops) *limit_stops = c[kBcLimitStops];
  if (suspended) *suspended = susp;
  return AGX_OK;
}

agx_status agx_read_backoff(agx_engine* e, uint64_t actor_id, uint32_t* suspended_for, uint32_t* until) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  uint32_t u = 0;
  if (e->d_backoff) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(copy_sync(e, &u, e->d_backoff + bo_until_off(e->nb) + actor_id, 4, hipMemcpyDeviceToHost));
  }
  if (suspended_for) *suspended_for = (uint64_t)u > e->sv_ticks + 1ull ? (uint32_t)(u - 1ull - e->sv_ticks) : 0u;
  if (until) *until = u;
  return AGX_OK;
}

// AA/dungeon/Children.scala; TY/internal/adapter/ActorContextAdapter.scala:79-106
agx_status agx_set_children(agx_engine* e, const agx_child_region* regions, uint32_t n_regions, const agx_spawn_site* sites,
                            uint32_t n_sites) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->wd_slots) return set_err(AGX_EINVAL, "children need an engine with death watch (agx_set_death_watch first)");
  if (e->started) return set_err(AGX_ESTATE, "set children before the first agx_run");
  if (n_regions < 1u || n_regions > AGX_MAX_CHILD_REGIONS || !regions)
    return set_err(AGX_EINVAL, "children: %u regions (1..%u)", n_regions, AGX_MAX_CHILD_REGIONS);
  if (n_sites > AGX_MAX_SPAWN_SITES || (n_sites && !sites))
    return set_err(AGX_EINVAL, "children: %u spawn sites (0..%u)", n_sites, AGX_MAX_SPAWN_SITES);
  if (e->beh_ctl_tags)
    return set_err(AGX_EINVAL, "children: the compiled behaviours name message tag 0xFD or 0xFC, reserved for Create and Stop "
                   "envelopes");
  const uint64_t n = e->n_global;
  for (uint32_t i = 0; i < n_regions; ++i) {
    const agx_child_region& r = regions[i];
    const uint64_t p0 = r.first_parent, p1 = p0 + r.n_parents, c0 = r.first_child, c1 = c0 + (uint64_t)r.n_parents * r.max_children;
    if (!r.n_parents || !r.max_children || p1 > n || c1 > n)
      return set_err(AGX_EINVAL, "children: region %u is empty or leaves [0, n_actors)", i);
    if (p0 < c1 && c0 < p1) return set_err(AGX_EINVAL, "children: region %u's child block overlaps its own parent range", i);
    for (uint32_t j = 0; j < i; ++j) {
      const agx_child_region& q = regions[j];
      const uint64_t q0 = q.first_parent, q1 = q0 + q.n_parents, d0 = q.first_child, d1 = d0 + (uint64_t)q.n_parents * q.max_children;
      if (p0 < q1 && q0 < p1) return set_err(AGX_EINVAL, "children: the parent ranges of regions %u and %u overlap", j, i);
      if (c0 < d1 && d0 < c1) return set_err(AGX_EINVAL, "children: the child blocks of regions %u and %u overlap", j, i);
    }
    for (uint64_t x = c0; x < c1; ++x)
      if (e->h_alive[x] & 1u)
        return set_err(AGX_EINVAL, "children: id %llu of region %u's child block is registered", (unsigned long long)x, i);
  }
  for (uint32_t i = 0; i < n_sites; ++i)
    if (sites[i].kind < AGX_KIND_COMPILED || sites[i].kind >= AGX_KIND_COMPILED + AGX_MAX_BEHAVIORS || (sites[i].flags & ~AGX_SITE_WORD1_PARENT))
      return set_err(AGX_EINVAL, "children: spawn site %u: kind %u is no compiled behaviour kind, or unknown flags", i, sites[i].kind);
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));
  AGX_TRY(alloc_watch(e));
  const size_t total = child_words(e);
  if (!e->d_child && hipMalloc((void**)&e->d_child, total * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_child = nullptr;
    return set_err(AGX_ENOMEM, "the child storage of %llu actors does not fit on the device", (unsigned long long)n);
  }
  std::vector<uint32_t> h(kCdBucketOff, 0u);
  h[0] = n_regions;
  h[1] = n_sites;
  for (uint32_t i = 0; i < n_regions; ++i) {
    h[kCdRegionOff + 4 * i] = regions[i].first_parent;
    h[kCdRegionOff + 4 * i + 1] = regions[i].n_parents;
    h[kCdRegionOff + 4 * i + 2] = regions[i].first_child;
    h[kCdRegionOff + 4 * i + 3] = regions[i].max_children;
  }
  for (uint32_t i = 0; i < n_sites; ++i) {
    uint32_t* S = &h[kCdSiteOff + 8 * i];
    S[0] = sites[i].kind;
    S[1] = sites[i].flags;
    S[2] = (uint32_t)sites[i].base0;
    S[3] = (uint32_t)(sites[i].base0 >> 32);
    S[4] = (uint32_t)sites[i].word1;
    S[5] = (uint32_t)(sites[i].word1 >> 32);
  }
  HIP_TRY(hipMemsetAsync(e->d_child, 0, total * 4ull, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_child, h.data(), h.size() * 4ull, hipMemcpyHostToDevice, e->stream));
  const unsigned long long addr = (unsigned long long)(uintptr_t)e->d_child;
  HIP_TRY(hipMemcpyAsync(e->d_watch + kWdChildPtr, &addr, 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (uint32_t i = 0; i < n_regions; ++i) {  // death tick "none" for the child blocks, once
    const uint32_t cnt = regions[i].n_parents * regions[i].max_children;
    hipLaunchKernelGGL(k_child_init, dim3((cnt + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream, e->d_watch, e->nb, e->bb,
                       regions[i].first_child, cnt);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ch_regions.assign(regions, regions + n_regions);
  e->ch_sites.assign(sites, sites + n_sites);
  e->ch_spawns.clear();
  e->ch_bad_spawn = false;
  if (!(e->kinds_mask & kb(AGX_KIND_COMPILED))) e->kinds_mask |= kb(AGX_KIND_COMPILED);  // (the children's kinds)
  drop_graphs(e);  // the variant is captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_spawn_children(agx_engine* e, uint64_t first_parent, uint64_t count, uint32_t site, uint32_t arg) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_child) {
    e->ch_bad_spawn = true;  // (agx_run refuses too: the rule of agx_start_watch)
    return set_err(AGX_EINVAL, "agx_spawn_children needs an engine with children (agx_set_children)");
  }
  if (first_parent + count > e->n_global || first_parent + count < first_parent) return set_err(AGX_EINVAL, "bad actor range");
  if (site >= e->ch_sites.size()) return set_err(AGX_EINVAL, "spawn site %u of %zu", site, e->ch_sites.size());
  if (arg > AGX_SPAWN_ARG_MASK) return set_err(AGX_EINVAL, "a spawn argument has %u bits", AGX_SPAWN_ARG_BITS);
  e->ch_spawns.push_back({first_parent, count, site, arg});
  return AGX_OK;
}

// the recorded host spawns take effect now (the actors' flags reach the device first when they are the newer ones)
static agx_status child_flush_now(agx_engine* e) {
  if (e->ch_spawns.empty()) return AGX_OK;
  AGX_TRY(flush_watch_starts(e));
  return flush_child_spawns(e);
}

agx_status agx_children_info(agx_engine* e, uint64_t* spawned, uint64_t* refused, uint64_t* created, uint64_t* child_stops,
                             uint64_t* cascade_stops, uint64_t* illegal_stops, uint64_t* discarded, uint64_t* live) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nl = 0;
  if (e->d_child) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(child_flush_now(e));
    AGX_TRY(copy_sync(e, c, e->d_child + kCdCtr, sizeof(c), hipMemcpyDeviceToHost));
    std::vector<uint32_t> lv(e->nb);
    AGX_TRY(copy_sync(e, lv.data(), e->d_child + kCdBucketOff, e->nb * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < e->nb; ++b) nl += lv[b];
  }
  if (spawned) *spawned = c[kCcSpawned];
  if (refused) *refused = c[kCcRefused];
  if (created) *created = c[kCcCreated];
  if (child_stops) *child_stops = c[kCcChildStops];
  if (cascade_stops) *cascade_stops = c[kCcCascade];
  if (illegal_stops) *illegal_stops = c[kCcIllegal];
  if (discarded) *discarded = c[kCcDiscarded];
  if (live) *live = nl;
  return AGX_OK;
}

agx_status agx_read_children(agx_engine* e, uint64_t actor_id, uint32_t* parent, uint32_t* spawn_count, uint32_t* created) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (actor_id >= e->n_global) return set_err(AGX_EINVAL, "bad actor id");
  uint32_t par = kWdNone, w = 0;
  for (const auto& r : e->ch_regions) {
    const uint64_t c0 = r.first_child, c1 = c0 + (uint64_t)r.n_parents * r.max_children;
    if (actor_id >= c0 && actor_id < c1) par = r.first_parent + (uint32_t)((actor_id - c0) / r.max_children);
  }
  if (e->d_child) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(child_flush_now(e));
    AGX_TRY(copy_sync(e, &w, e->d_child + cd_count_off(e->nb) + actor_id, 4, hipMemcpyDeviceToHost));
  }
  if (parent) *parent = par;
  if (spawn_count) *spawn_count = w & ~kCdCreated;
  if (created) *created = (w & kCdCreated) ? 1u : 0u;
  return AGX_OK;
}

// TY/internal/receptionist/LocalReceptionist.scala:147-248; TY/internal/routing/GroupRouterImpl.scala:114-146
agx_status agx_set_receptionist(agx_engine* e, uint32_t n_keys, uint32_t capacity) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (n_keys < 1u || n_keys > AGX_MAX_SERVICE_KEYS || capacity < 1u)
    return set_err(AGX_EINVAL, "the receptionist: %u service keys (1..%u), listings of %u ids (at least 1)", n_keys,
                   AGX_MAX_SERVICE_KEYS, capacity);
  if (e->d_recep) return set_err(AGX_EINVAL, "the receptionist is already set (%u service keys)", e->rc_keys);
  AGX_TRY(refuse_feature(e, F_RECEP));
  AGX_TRY(ensure_dev(e));
  const uint32_t cap = (uint32_t)std::min<uint64_t>(capacity, e->n_global);  // (a listing never holds more ids than there are)
  const size_t words = rc_mask_off(n_keys, cap, e->nb) + (((size_t)e->nb << e->bb) + 3u) / 4u;
  if (hipMalloc((void**)&e->d_recep, words * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_recep = nullptr;
    return set_err(AGX_ENOMEM, "the receptionist's storage (%u keys, listings of %u ids, %llu actors: %llu MB) does not fit "
                   "on the device", n_keys, cap, (unsigned long long)e->n_global, (unsigned long long)(words >> 18));
  }
  const uint32_t head[3] = {n_keys, cap, e->nb};
  HIP_TRY(hipMemsetAsync(e->d_recep, 0, words * 4ull, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_recep, head, sizeof(head), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->rc_keys = n_keys;
  e->rc_cap = cap;
  e->rc_starts.clear();
  e->rc_bad_start = false;
  drop_graphs(e);  // the variant, the storage and the rebuild kernels are captured in the superstep graphs
  return AGX_OK;
}

// TY/internal/pubsub/TopicImpl.scala:60-143
agx_status agx_set_topics(agx_engine* e, uint32_t log_capacity) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (log_capacity < 1u || log_capacity > AGX_MAX_TOPIC_LOG)
    return set_err(AGX_EINVAL, "topics: a log of %u publications per tick (1..%u)", log_capacity, AGX_MAX_TOPIC_LOG);
  if (e->d_topic) return set_err(AGX_EINVAL, "topics are already set (a log of %u publications)", e->tp_cap);
  if (!e->d_recep)
    return set_err(AGX_EINVAL, "topics need an engine with the receptionist (agx_set_receptionist): a topic is a service key");
  if (e->d_hash)
    return set_err(AGX_EINVAL, "topics need an engine without router logics (agx_set_router_logics): the hashed and random "
                   "routes know no topics");
  if (e->started) return set_err(AGX_ESTATE, "set topics before the first agx_run");
  AGX_TRY(ensure_dev(e));
  const size_t words = tp_words(log_capacity, e->nb);
  if (hipMalloc((void**)&e->d_topic, words * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_topic = nullptr;
    return set_err(AGX_ENOMEM, "the topics' storage (a log of %u publications, %u buckets: %llu KB) does not fit on the device",
                   log_capacity, e->nb, (unsigned long long)(words >> 8));
  }
  const uint32_t head[2] = {log_capacity, e->nb};
  const unsigned long long addr = (unsigned long long)(uintptr_t)e->d_topic;
  HIP_TRY(hipMemsetAsync(e->d_topic, 0, words * 4ull, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_topic, head, sizeof(head), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_recep + kRcTopicPtr, &addr, sizeof(addr), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->tp_cap = log_capacity;
  e->tp_pubs.clear();
  drop_graphs(e);  // the variant, the storage and the plan kernel are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_publish(agx_engine* e, uint32_t key, uint32_t sender, uint32_t payload) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_topic) return set_err(AGX_EINVAL, "agx_publish needs an engine with topics (agx_set_topics)");
  if (key >= e->rc_keys) return set_err(AGX_EINVAL, "topic %u of %u", key, e->rc_keys);
  e->tp_pubs.push_back({key, sender, payload});
  return AGX_OK;
}

agx_status agx_topic_info(agx_engine* e, uint64_t* published, uint64_t* fanned_out, uint64_t* no_subscribers,
                          uint64_t* host_published) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint64_t c[4] = {0, 0, 0, 0};
  if (e->d_topic) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_recep_starts(e));
    AGX_TRY(copy_sync(e, c, e->d_topic + kTpCtr, sizeof(c), hipMemcpyDeviceToHost));
  }
  if (published) *published = c[kTpPublished];
  if (fanned_out) *fanned_out = c[kTpFannedOut];
  if (no_subscribers) *no_subscribers = c[kTpNoSubscribers];
  if (host_published) *host_published = c[kTpHostPublished];
  return AGX_OK;
}

agx_status agx_read_topic_log(agx_engine* e, uint32_t* out_key, uint32_t* out_sender, uint32_t* out_payload, uint64_t cap,
                              uint64_t* out_n) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_topic) return set_err(AGX_EINVAL, "agx_read_topic_log needs an engine with topics (agx_set_topics)");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  uint32_t n = 0;
  AGX_TRY(copy_sync(e, &n, e->d_topic + kTpNLog, 4, hipMemcpyDeviceToHost));
  n = std::min(n, e->tp_cap);
  const uint64_t take = std::min<uint64_t>(n, cap);
  if (take) {
    std::vector<uint32_t> lg(take * 4ull);
    AGX_TRY(copy_sync(e, lg.data(), e->d_topic + tp_log_off(e->nb), take * 16ull, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < take; ++i) {
      if (out_key) out_key[i] = lg[4 * i];
      if (out_sender) out_sender[i] = lg[4 * i + 1];
      if (out_payload) out_payload[i] = lg[4 * i + 2];
    }
  }
  if (out_n) *out_n = n;
  return AGX_OK;
}

// TY/internal/receptionist/LocalReceptionist.scala:152-171,209-220,233-238
agx_status agx_set_listings(agx_engine* e, const uint32_t* listing_payload, uint32_t n_keys) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!listing_payload) return set_err(AGX_EINVAL, "listings: null listing_payload");
  if (e->d_list) return set_err(AGX_EINVAL, "listings are already set (%u keys)", e->rc_keys);
  if (!e->d_topic)
    return set_err(AGX_EINVAL, "listings need an engine with topics (agx_set_topics after agx_set_receptionist): a Listing "
                   "is injected as a publication's delivery is");
  if (n_keys != e->rc_keys)
    return set_err(AGX_EINVAL, "listings: %u Listing payloads, but the receptionist has %u keys (agx_set_receptionist)", n_keys,
                   e->rc_keys);
  if (e->started) return set_err(AGX_ESTATE, "set listings before the first agx_run");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));  // (what the host registered before this call is no change a subscriber is told of)
  const size_t words = ls_words(n_keys, e->nb, e->bb);
  if (hipMalloc((void**)&e->d_list, words * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_list = nullptr;
    return set_err(AGX_ENOMEM, "the listings' storage (%u keys, %u buckets: %llu KB) does not fit on the device", n_keys, e->nb,
                   (unsigned long long)(words >> 8));
  }
  const uint32_t head[3] = {n_keys, e->nb, e->bb};
  const unsigned long long addr = (unsigned long long)(uintptr_t)e->d_list;
  hipError_t he = hipMemsetAsync(e->d_list, 0, words * 4ull, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_list, head, sizeof(head), hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_list + kLsPayload, listing_payload, 4ull * n_keys, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_recep + kRcListPtr, &addr, sizeof(addr), hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  if (he != hipSuccess) {  // (no half-set listings: the engine stays one without them, and the call may be repeated)
    const unsigned long long none = 0ull;
    (void)hipMemcpy(e->d_recep + kRcListPtr, &none, sizeof(none), hipMemcpyHostToDevice);
    (void)hipFree(e->d_list);
    e->d_list = nullptr;
    HIP_TRY(he);
  }
  e->ls_starts.clear();
  drop_graphs(e);  // the variant, the storage and the plan kernel are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_subscribe_listings(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t key, uint32_t on) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_list) return set_err(AGX_EINVAL, "agx_subscribe_listings needs an engine with listings (agx_set_listings)");
  if (key >= e->rc_keys) return set_err(AGX_EINVAL, "service key %u of %u", key, e->rc_keys);
  if (first_id > e->n_local || count > e->n_local - first_id)
    return set_err(AGX_EINVAL, "actors [%llu, %llu) of %llu", (unsigned long long)first_id,
                   (unsigned long long)(first_id + count), (unsigned long long)e->n_local);
  e->ls_starts.push_back({first_id, count, key, on ? 1u : 0u});
  return AGX_OK;
}

agx_status agx_listing_info(agx_engine* e, uint64_t* subscribes, uint64_t* finds, uint64_t* listings_sent, uint64_t* notified) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_list) return set_err(AGX_EINVAL, "agx_listing_info needs an engine with listings (agx_set_listings)");
  uint64_t c[4] = {0, 0, 0, 0};
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  AGX_TRY(copy_sync(e, c, e->d_list + kLsCtr, sizeof(c), hipMemcpyDeviceToHost));
  if (subscribes) *subscribes = c[kLsSubscribes];
  if (finds) *finds = c[kLsFinds];
  if (listings_sent) *listings_sent = c[kLsSent];
  if (notified) *notified = c[kLsNotified];
  return AGX_OK;
}

agx_status agx_read_subscriptions(agx_engine* e, uint64_t first, uint64_t count, uint8_t* sub_out, uint8_t* pending_out) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_list) return set_err(AGX_EINVAL, "agx_read_subscriptions needs an engine with listings (agx_set_listings)");
  if (first > e->n_local || count > e->n_local - first)
    return set_err(AGX_EINVAL, "actors [%llu, %llu) of %llu", (unsigned long long)first, (unsigned long long)(first + count),
                   (unsigned long long)e->n_local);
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  if (!count) return AGX_OK;
  const uint8_t* const sub = reinterpret_cast<const uint8_t*>(e->d_list + ((ls_mask_off(e->rc_keys, e->nb) + 3u) & ~(size_t)3));
  if (sub_out) AGX_TRY(copy_sync(e, sub_out, sub + first, count, hipMemcpyDeviceToHost));
  if (pending_out) AGX_TRY(copy_sync(e, pending_out, sub + ((size_t)e->nb << e->bb) + first, count, hipMemcpyDeviceToHost));
  return AGX_OK;
}

// TY/internal/routing/RoutingLogic.scala:77-112; akka-actor routing/ConsistentHash.scala:25-139
agx_status agx_set_router_logics(agx_engine* e, uint32_t hashed_keys_mask, uint32_t virtual_nodes_factor, uint64_t seed) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_recep)
    return set_err(AGX_EINVAL, "router logics need an engine with the receptionist (agx_set_receptionist): a router routes "
                   "through a service key");
  if (e->d_topic)
    return set_err(AGX_EINVAL, "router logics need an engine without topics (agx_set_topics): the hashed and random routes "
                   "know no topics");
  if (e->d_hash) return set_err(AGX_EINVAL, "router logics are already set (hashed_keys_mask 0x%x)", e->hr_mask);
  if (hashed_keys_mask >> e->rc_keys)
    return set_err(AGX_EINVAL, "router logics: hashed_keys_mask 0x%x names a service key past the receptionist's %u",
                   hashed_keys_mask, e->rc_keys);
  if (hashed_keys_mask && (virtual_nodes_factor < 1u || virtual_nodes_factor > AGX_MAX_VIRTUAL_NODES))
    return set_err(AGX_EINVAL, "router logics: a virtual_nodes_factor of %u (1..%u)", virtual_nodes_factor, AGX_MAX_VIRTUAL_NODES);
  if (hashed_keys_mask && e->n_global * (uint64_t)virtual_nodes_factor > AGX_MAX_RING_POINTS)
    return set_err(AGX_EINVAL, "router logics: %llu actors x a virtual_nodes_factor of %u are more than %u ring points",
                   (unsigned long long)e->n_global, virtual_nodes_factor, AGX_MAX_RING_POINTS);
  if (e->started) return set_err(AGX_ESTATE, "set router logics before the first agx_run");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));  // (what was registered before this call is in the first rings: no ring_rebuilds for it)
  const uint32_t factor = hashed_keys_mask ? virtual_nodes_factor : 0u;
  const uint32_t npts = (uint32_t)(e->n_global * factor), nseg = (npts + kHrSeg - 1u) / kHrSeg;
  const uint32_t nslots = (uint32_t)__builtin_popcount(hashed_keys_mask);
  const size_t words = hr_words(nslots, nseg, npts);
  // the ring of all actors, built once on the host: every id's points, sorted by (signed hash, id)
  std::vector<uint64_t> pts(npts);
  for (uint64_t a = 0; a < (npts ? e->n_global : 0); ++a) {
    const uint32_t nh = mm_decimal_hash((uint32_t)a);
    for (uint32_t v = 1; v <= factor; ++v)
      pts[a * factor + v - 1u] = ((uint64_t)(mm_node_point(nh, v) ^ 0x80000000u) << 32) | a;  // (the sign bit flipped: signed order)
  }
  std::sort(pts.begin(), pts.end());
  std::vector<uint32_t> st(2ull * npts);
  for (uint32_t i = 0; i < npts; ++i) {
    st[i] = (uint32_t)(pts[i] >> 32) ^ 0x80000000u;
    st[npts + i] = (uint32_t)pts[i];
  }
  if (hipMalloc((void**)&e->d_hash, words * 4ull) != hipSuccess) {
    (void)hipGetLastError();
    e->d_hash = nullptr;
    return set_err(AGX_ENOMEM, "the hash rings' storage (%u hashed keys, %u ring points: %llu MB) does not fit on the device",
                   nslots, npts, (unsigned long long)(words >> 18));
  }
  uint32_t head[6] = {hashed_keys_mask, factor, npts, nseg, (uint32_t)seed, (uint32_t)(seed >> 32)};
  const unsigned long long addr = (unsigned long long)(uintptr_t)e->d_hash;
  hipError_t he = hipMemsetAsync(e->d_hash, 0, words * 4ull, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_hash, head, sizeof(head), hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess && npts)
    he = hipMemcpyAsync(e->d_hash + hr_static_off(nslots, nseg), st.data(), st.size() * 4ull, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(e->d_recep + kRcHashPtr, &addr, sizeof(addr), hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);  // (`st` and `head` are read until here)
  if (he != hipSuccess) {
    const unsigned long long none = 0ull;
    (void)hipMemcpy(e->d_recep + kRcHashPtr, &none, sizeof(none), hipMemcpyHostToDevice);
    (void)hipFree(e->d_hash);
    e->d_hash = nullptr;
    HIP_TRY(he);
  }
  e->hr_mask = hashed_keys_mask;
  e->hr_factor = factor;
  e->hr_npts = npts;
  e->hr_nseg = nseg;
  launch_hash_rebuild(e, hashed_keys_mask);  // (the rings of what is registered already)
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  drop_graphs(e);  // the variant, the storage and the ring kernels are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_router_info(agx_engine* e, uint64_t* hashed, uint64_t* random, uint64_t* ring_rebuilds, uint32_t ring_size[8]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint32_t h[kHrSegOff] = {0};
  if (e->d_hash) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_recep_starts(e));
    AGX_TRY(copy_sync(e, h, e->d_hash, sizeof(h), hipMemcpyDeviceToHost));
  }
  uint64_t c[3];
  memcpy(c, h + kHrCtr, sizeof(c));
  if (hashed) *hashed = c[kHrHashed];
  if (random) *random = c[kHrRandom];
  if (ring_rebuilds) *ring_rebuilds = c[kHrRebuilds];
  for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k)
    if (ring_size) ring_size[k] = h[kHrSize + k];
  return AGX_OK;
}

agx_status agx_read_hash_ring(agx_engine* e, uint32_t key, uint32_t* out_hash, uint32_t* out_id, uint64_t cap, uint64_t* out_n) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_hash) return set_err(AGX_EINVAL, "agx_read_hash_ring needs an engine with router logics (agx_set_router_logics)");
  if (key >= AGX_MAX_SERVICE_KEYS || !((e->hr_mask >> key) & 1u))
    return set_err(AGX_EINVAL, "service key %u is not a hashed key (hashed_keys_mask 0x%x)", key, e->hr_mask);
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  uint32_t n = 0;
  AGX_TRY(copy_sync(e, &n, e->d_hash + kHrSize + key, 4, hipMemcpyDeviceToHost));
  n = std::min(n, e->hr_npts);
  const uint64_t take = std::min<uint64_t>(n, cap);
  const uint32_t nslots = (uint32_t)__builtin_popcount(e->hr_mask), sl = (uint32_t)__builtin_popcount(e->hr_mask & ((1u << key) - 1u));
  const uint32_t* const ring = e->d_hash + hr_static_off(nslots, e->hr_nseg) + 2ull * e->hr_npts * (1ull + sl);
  if (take && out_hash) AGX_TRY(copy_sync(e, out_hash, ring, take * 4ull, hipMemcpyDeviceToHost));
  if (take && out_id) AGX_TRY(copy_sync(e, out_id, ring + e->hr_npts, take * 4ull, hipMemcpyDeviceToHost));
  if (out_n) *out_n = n;
  return AGX_OK;
}

agx_status agx_register_services(agx_engine* e, uint64_t first_id, uint64_t count, uint32_t key, uint32_t on) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_recep) {
    e->rc_bad_start = true;  // (agx_run refuses too: the rule of agx_start_watch)
    return set_err(AGX_EINVAL, "agx_register_services needs an engine with the receptionist (agx_set_receptionist)");
  }
  if (first_id + count > e->n_global || first_id + count < first_id) return set_err(AGX_EINVAL, "bad actor range");
  if (key >= e->rc_keys) return set_err(AGX_EINVAL, "service key %u of %u", key, e->rc_keys);
  e->rc_starts.push_back({first_id, count, key, on ? 1u : 0u});
  return AGX_OK;
}

agx_status agx_read_listing(agx_engine* e, uint32_t key, uint32_t* out_ids, uint64_t cap, uint64_t* out_n) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_recep) return set_err(AGX_EINVAL, "agx_read_listing needs an engine with the receptionist (agx_set_receptionist)");
  if (key >= e->rc_keys) return set_err(AGX_EINVAL, "service key %u of %u", key, e->rc_keys);
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  uint32_t n = 0;
  AGX_TRY(copy_sync(e, &n, e->d_recep + kRcSize + key, 4, hipMemcpyDeviceToHost));
  const uint64_t take = std::min<uint64_t>(n, out_ids ? cap : 0);
  if (take)
    AGX_TRY(copy_sync(e, out_ids, e->d_recep + rc_list_off(e->rc_keys, e->nb) + (size_t)key * e->rc_cap, take * 4ull,
                      hipMemcpyDeviceToHost));
  if (out_n) *out_n = n;
  return AGX_OK;
}

agx_status agx_read_services(agx_engine* e, uint64_t first, uint64_t count, uint8_t* out_masks) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!e->d_recep) return set_err(AGX_EINVAL, "agx_read_services needs an engine with the receptionist (agx_set_receptionist)");
  if (first + count > e->n_global || first + count < first || (count && !out_masks)) return set_err(AGX_EINVAL, "bad actor range");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(flush_recep_starts(e));
  if (count)
    AGX_TRY(copy_sync(e, out_masks, reinterpret_cast<const uint8_t*>(e->d_recep + rc_mask_off(e->rc_keys, e->rc_cap, e->nb)) + first,
                      count, hipMemcpyDeviceToHost));
  return AGX_OK;
}

agx_status agx_receptionist_info(agx_engine* e, uint64_t* routed, uint64_t* no_routees, uint64_t* registered,
                                 uint64_t* deregistered, uint64_t* terminated, uint64_t* rebuilds, uint32_t size[8],
                                 uint64_t version[8]) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  uint32_t h[kRcCntOff] = {0};
  if (e->d_recep) {
    AGX_TRY(ensure_dev(e));
    AGX_TRY(flush_recep_starts(e));
    AGX_TRY(copy_sync(e, h, e->d_recep, sizeof(h), hipMemcpyDeviceToHost));
  }
  uint64_t c[6], v[8];
  memcpy(c, h + kRcCtr, sizeof(c));
  memcpy(v, h + kRcVersion, sizeof(v));
  if (routed) *routed = c[kRcRouted];
  if (no_routees) *no_routees = c[kRcNoRoutees];
  if (registered) *registered = c[kRcRegistered];
  if (deregistered) *deregistered = c[kRcDeregistered];
  if (terminated) *terminated = c[kRcTerminated];
  if (rebuilds) *rebuilds = c[kRcRebuilds];
  for (uint32_t k = 0; k < AGX_MAX_SERVICE_KEYS; ++k) {
    if (size) size[k] = h[kRcSize + k];
    if (version) version[k] = v[k];
  }
  return AGX_OK;
}

agx_status agx_set_outbound(agx_engine* e, uint32_t first_host_id, uint32_t n_host, uint64_t capacity) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (n_host && (first_host_id < e->n_global || (uint64_t)first_host_id + n_host > (1ull << 31)))
    return set_err(AGX_EINVAL, "host ids must lie in [n_actors, 2^31) (bit 31 of a sender tags CRDT state gossips)");
  if (n_host && (capacity == 0 || capacity > 0x3FFFFFFFull))
    return set_err(AGX_EINVAL, "outbox capacity must be in [1, 2^30)");
  AGX_TRY(ensure_dev(e));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (!e->d_outbox_n) {
    AGX_TRY(dalloc(&e->d_outbox_n, 1));
    HIP_TRY(hipMemsetAsync(e->d_outbox_n, 0, 4, e->stream));
  }
  if (n_host && capacity != e->outbox_cap) {
    AGX_TRY(drain_outbox(e));  // tells still in the old buffer move to the host queue first
    hipFree(e->d_outbox);
    e->d_outbox = nullptr;
    AGX_TRY(dalloc(&e->d_outbox, 3 * capacity));
    e->outbox_cap = capacity;
  }
  HIP_TRY(hipDeviceSynchronize());  // (null-stream allocation / memset before the engine stream uses them)
  e->host_lo = first_host_id;
  e->host_n = n_host;
  drop_graphs(e);  // the host-id range is a kernel parameter captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_take_outbound(agx_engine* e, uint32_t* dst, uint32_t* src, uint32_t* payload, uint64_t cap,
                             uint64_t* n) {
  if (!e || !n || (cap && (!dst || !src || !payload))) return set_err(AGX_EINVAL, "bad take_outbound args");
  *n = 0;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(drain_outbox(e));
  if (e->outbox_lost) {  // reported once, then cleared: the engine stays usable after an overflow
    const uint64_t lost = e->outbox_lost;
    e->outbox_lost = 0;
    return set_err(AGX_ECAPACITY, "%llu outbound tells dropped: more than the outbox capacity %llu between two "
                   "agx_take_outbound calls", (unsigned long long)lost, (unsigned long long)e->outbox_cap);
  }
  const uint64_t k = std::min<uint64_t>(cap, e->outq.size() / 3);
  for (uint64_t i = 0; i < k; ++i) {
    dst[i] = e->outq[3 * i];
    src[i] = e->outq[3 * i + 1];
    payload[i] = e->outq[3 * i + 2];
  }
  e->outq.erase(e->outq.begin(), e->outq.begin() + 3 * k);
  *n = k;
  return AGX_OK;
}

agx_status agx_set_gossip(agx_engine* e, uint32_t fanout, uint64_t seed) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (fanout + 1 > e->kmax) return set_err(AGX_EINVAL, "gossip fanout %u needs max_emit >= %u", fanout, fanout + 1);
  e->gossip_f = fanout;
  e->gossip_seed = seed;
  drop_graphs(e);  // behaviour parameters are captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_set_behaviors(agx_engine* e, const agx_case* cases, uint32_t n_cases, const agx_act* acts,
                             uint32_t n_acts, const uint32_t* first, uint32_t n_beh) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (e->started) return set_err(AGX_ESTATE, "set compiled behaviours before agx_run");
  if (n_beh == 0 || n_beh > AGX_MAX_BEHAVIORS || n_cases > AGX_MAX_CASES || n_acts > AGX_MAX_ACTS || !first ||
      (n_cases && !cases) || (n_acts && !acts))
    return set_err(AGX_EINVAL, "compiled behaviours: bad table sizes");
  if (first[0] != 0 || first[n_beh] != n_cases) return set_err(AGX_EINVAL, "first[] must run from 0 to n_cases");
  for (uint32_t b = 0; b < n_beh; ++b)
    if (first[b] > first[b + 1]) return set_err(AGX_EINVAL, "first[] must be non-decreasing");
  auto opnd_ok = [](uint32_t src, uint32_t word) {
    if (src == AGX_V_SPAWNED) return word <= 1u;
    if (src == AGX_V_CHILD) return word <= AGX_CHILD_NO_WORD;
    if (src == AGX_V_LISTING_SIZE) return word < AGX_MAX_SERVICE_KEYS;
    if (src == AGX_V_SERVICE_AT) return word < (AGX_MAX_SERVICE_KEYS << 2);
    return src == AGX_V_TIMER ? word < AGX_MAX_TIMER_KEYS : src <= AGX_V_STASH && word <= 1u;
  };
  // a supervision signal case (include/akka_gpu.h AGX_SIGNAL_PRERESTART): a signal case whose first test is
  // payload == PreRestart / PostStop; every other signal case is death watch's
  auto sv_signal = [](const agx_case& C) {
    return (C.result & AGX_CASE_SIGNAL) && C.src1 == AGX_V_PAYLOAD && C.k1 == 0 && C.cmp1 == AGX_CMP_EQ &&
           C.src2 == AGX_V_CONST && (C.k2 == (int64_t)AGX_SIGNAL_PRERESTART || C.k2 == (int64_t)AGX_SIGNAL_POSTSTOP);
  };
  for (uint32_t c = 0; c < n_cases; ++c) {
    agx_case C = cases[c];
    if (C.result & AGX_CASE_SIGNAL) {  // a signal case (death watch): same, stopped, unhandled or become
      C.result &= (uint8_t)~AGX_CASE_SIGNAL;
      if (sv_signal(cases[c]) && C.result != AGX_RES_SAME)
        return set_err(AGX_EINVAL, "compiled behaviours: PreRestart / PostStop signal case %u must end in same", c);
      if (C.result > AGX_RES_BECOME) return set_err(AGX_EINVAL, "compiled behaviours: signal case %u stashes, unstashes or fails", c);
    }
    if (!opnd_ok(C.src1, C.word1) || !opnd_ok(C.src2, C.word2) || !opnd_ok(C.src3, C.word3) ||
        !opnd_ok(C.src4, C.word4) || C.cmp1 > AGX_CMP_GE || C.cmp2 > AGX_CMP_GE || C.result > AGX_RES_FAIL ||
        (C.result == AGX_RES_FAIL && C.next >= AGX_MAX_EXCEPTION_CLASSES) ||
        (C.result == AGX_RES_BECOME && C.next >= n_beh) ||
        (C.result == AGX_RES_UNSTASH_ALL && C.next >= n_beh && C.next != AGX_NEXT_SAME) || (uint32_t)C.act_first + C.act_count > n_acts)
      return set_err(AGX_EINVAL, "compiled behaviours: bad case %u", c);
  }
  for (uint32_t i = 0; i < n_acts; ++i) {
    const agx_act& A = acts[i];
    const bool askop = A.op == AGX_A_ASK_ARM || A.op == AGX_A_ASK_SEND;  // (`word` is the key)
    const bool tmop = (A.op >= AGX_A_TIMER_SINGLE && A.op <= AGX_A_TIMER_CANCEL_ALL) || askop;  // (`word` is the key)
    const bool wdop = A.op >= AGX_A_WATCH && A.op <= AGX_A_UNWATCH;  // (the ref is the d-operand)
    const bool rcop = (A.op >= AGX_A_REGISTER && A.op <= AGX_A_ROUTE) || (A.op >= AGX_A_PUBLISH && A.op <= AGX_A_FIND);  // (`pad1` is the service key)
    constexpr uint32_t kRouteFlags = AGX_ROUTE_KEEP_SENDER | AGX_ROUTE_BY_INDEX | AGX_ROUTE_HASHED | AGX_ROUTE_RANDOM;
    if (rcop && A.op == AGX_A_ROUTE && A.pad1 < AGX_MAX_SERVICE_KEYS && A.pad0 > (AGX_ROUTE_KEEP_SENDER | AGX_ROUTE_BY_INDEX) &&
        (A.pad0 > kRouteFlags || ((A.pad0 & (AGX_ROUTE_BY_INDEX | AGX_ROUTE_HASHED)) && !opnd_ok(A.dsrc, A.dword))))
      return set_err(AGX_EINVAL, "compiled behaviours: bad action %u (service keys 0..7, route flags 0..15)", i);
    if (rcop && (A.pad1 >= AGX_MAX_SERVICE_KEYS || A.pad0 > (A.op == AGX_A_ROUTE ? kRouteFlags : 0u) ||
                 (A.op == AGX_A_ROUTE && (A.pad0 & AGX_ROUTE_BY_INDEX) && !opnd_ok(A.dsrc, A.dword))))
      return set_err(AGX_EINVAL, "compiled behaviours: bad action %u (service keys 0..7, route flags 0..3)", i);
    if (A.op < AGX_A_SET || A.op > AGX_A_PASSIVATE || A.word > (tmop ? AGX_MAX_TIMER_KEYS - 1u : 1u) ||
        !opnd_ok(A.src, A.sword) ||
        ((A.op == AGX_A_TELL || A.op == AGX_A_TIMER_SINGLE || A.op == AGX_A_TIMER_PERIODIC || wdop || A.op == AGX_A_STOP_CHILD ||
          A.op == AGX_A_SET_RECEIVE_TIMEOUT || askop) &&
         !opnd_ok(A.dsrc, A.dword)) ||
        (A.op == AGX_A_ASK_ARM && A.pad0 > 1u) ||
        (A.op == AGX_A_SPAWN && A.dword >= AGX_MAX_SPAWN_SITES))
      return set_err(AGX_EINVAL, "compiled behaviours: bad action %u (state words 0..1, timer keys 0..3, spawn sites 0..63)", i);
  }
  for (uint32_t i = 0; i < n_acts; ++i)
    if (acts[i].op == AGX_A_SET_RECEIVE_TIMEOUT && acts[i].dsrc == AGX_V_CONST && acts[i].dk < 1)
      return set_err(AGX_EINVAL, "compiled behaviours: action %u sets a receive timeout of %lld ticks (a constant delay is at "
                     "least 1)", i, (long long)acts[i].dk);
  for (uint32_t i = 0; i < n_acts; ++i)
    if (acts[i].op == AGX_A_ASK_ARM && acts[i].dsrc == AGX_V_CONST && acts[i].dk < 1)
      return set_err(AGX_EINVAL, "compiled behaviours: action %u asks with a timeout of %lld ticks (a constant timeout is at "
                     "least 1)", i, (long long)acts[i].dk);
  // receive timeouts: tag 0xFB named by a tag test or a message tag (refused on an engine with receive timeouts)
  bool rt_tag = false;
  auto rt_named = [&](uint32_t s1, int64_t k1, uint32_t cmp, uint32_t s2, int64_t k2) {
    if (cmp == AGX_CMP_ANY) return;
    rt_tag |= s1 == AGX_V_TAG && k1 == 0 && s2 == AGX_V_CONST && k2 == (int64_t)AGX_TAG_RECEIVE_TIMEOUT;
    rt_tag |= s2 == AGX_V_TAG && k2 == 0 && s1 == AGX_V_CONST && k1 == (int64_t)AGX_TAG_RECEIVE_TIMEOUT;
  };
  for (uint32_t c = 0; c < n_cases; ++c) {
    rt_named(cases[c].src1, cases[c].k1, cases[c].cmp1, cases[c].src2, cases[c].k2);
    rt_named(cases[c].src3, cases[c].k3, cases[c].cmp2, cases[c].src4, cases[c].k4);
  }
  for (uint32_t i = 0; i < n_acts; ++i) rt_tag |= (acts[i].or_mask >> 24) == AGX_TAG_RECEIVE_TIMEOUT;
  if (e->rt_on && rt_tag)
    return set_err(AGX_EINVAL, "compiled behaviours: message tag 0xFB is reserved for receive-timeout envelopes on an engine "
                   "with receive timeouts");
  // children: a spawn and a stop of a child each send one envelope through the case's tell slot
  bool uses_child = false, ctl_tags = false;
  auto ch_use = [&](uint32_t src) { uses_child |= src == AGX_V_SPAWNED || src == AGX_V_CHILD; };
  auto tag_named = [&](uint32_t s1, int64_t k1, uint32_t cmp, uint32_t s2, int64_t k2) {
    if (cmp == AGX_CMP_ANY) return;
    ctl_tags |= s1 == AGX_V_TAG && k1 == 0 && s2 == AGX_V_CONST && (k2 == (int64_t)AGX_TAG_CREATE || k2 == (int64_t)AGX_TAG_STOP);
    ctl_tags |= s2 == AGX_V_TAG && k2 == 0 && s1 == AGX_V_CONST && (k1 == (int64_t)AGX_TAG_CREATE || k1 == (int64_t)AGX_TAG_STOP);
  };
  for (uint32_t c = 0; c < n_cases; ++c) {
    const agx_case& C = cases[c];
    ch_use(C.src1); ch_use(C.src2); ch_use(C.src3); ch_use(C.src4);
    tag_named(C.src1, C.k1, C.cmp1, C.src2, C.k2);
    tag_named(C.src3, C.k3, C.cmp2, C.src4, C.k4);
    uint32_t sends = 0;
    bool child_op = false;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      sends += acts[i].op == AGX_A_TELL || acts[i].op == AGX_A_SPAWN || acts[i].op == AGX_A_STOP_CHILD;
      child_op |= acts[i].op == AGX_A_SPAWN || acts[i].op == AGX_A_STOP_CHILD;
    }
    if (child_op && sends > 1u)
      return set_err(AGX_EINVAL, "compiled behaviours: case %u holds %u of tell, spawn and stop-child; an engine with children "
                     "has max_emit 1", c, sends);
  }
  for (uint32_t i = 0; i < n_acts; ++i) {
    ch_use(acts[i].src);
    ch_use(acts[i].dsrc);
    uses_child |= acts[i].op == AGX_A_SPAWN || acts[i].op == AGX_A_STOP_CHILD;
    const uint32_t t = acts[i].or_mask >> 24;
    ctl_tags |= t == AGX_TAG_CREATE || t == AGX_TAG_STOP;
  }
  if (e->d_child && ctl_tags)
    return set_err(AGX_EINVAL, "compiled behaviours: message tags 0xFD and 0xFC are reserved for Create and Stop envelopes on "
                   "an engine with children");
  // sharding: a Passivate sends the entity's stop message through the case's tell slot
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t sends = 0;
    bool pas = false;
    for (uint32_t i = cases[c].act_first; i < (uint32_t)cases[c].act_first + cases[c].act_count; ++i) {
      sends += acts[i].op == AGX_A_TELL || acts[i].op == AGX_A_PASSIVATE;
      pas |= acts[i].op == AGX_A_PASSIVATE;
    }
    if (pas && sends > 1u)
      return set_err(AGX_EINVAL, "compiled behaviours: case %u holds %u of tell and passivate; an engine with sharding has "
                     "max_emit 1", c, sends);
  }
  // the receptionist: a route sends one envelope through the case's tell slot; the service keys the tables use
  bool uses_recep = false, uses_publish = false, uses_listing = false;
  uint32_t rc_keys_used = 0;
  auto rc_use = [&](uint32_t src, uint32_t word) {
    if (src != AGX_V_LISTING_SIZE && src != AGX_V_SERVICE_AT) return;
    uses_recep = true;
    rc_keys_used = std::max(rc_keys_used, (word & 7u) + 1u);
  };
  for (uint32_t c = 0; c < n_cases; ++c) {
    const agx_case& C = cases[c];
    rc_use(C.src1, C.word1); rc_use(C.src2, C.word2); rc_use(C.src3, C.word3); rc_use(C.src4, C.word4);
    uint32_t sends = 0;
    bool route = false, publish = false;
    for (uint32_t i = C.act_first; i < (uint32_t)C.act_first + C.act_count; ++i) {
      sends += acts[i].op == AGX_A_TELL || acts[i].op == AGX_A_ROUTE || acts[i].op == AGX_A_PUBLISH;
      route |= acts[i].op == AGX_A_ROUTE;
      publish |= acts[i].op == AGX_A_PUBLISH;
    }
    if (publish && sends > 1u)
      return set_err(AGX_EINVAL, "compiled behaviours: case %u holds %u of tell, route and publish; an engine with topics has "
                     "max_emit 1", c, sends);
    if (route && sends > 1u)
      return set_err(AGX_EINVAL, "compiled behaviours: case %u holds %u of tell and route; an engine with the receptionist "
                     "has max_emit 1", c, sends);
  }
  for (uint32_t i = 0; i < n_acts; ++i) {
    rc_use(acts[i].src, acts[i].sword);
    rc_use(acts[i].dsrc, acts[i].dword);
    uses_publish |= acts[i].op == AGX_A_PUBLISH;
    uses_listing |= acts[i].op == AGX_A_SUBSCRIBE_LISTING || acts[i].op == AGX_A_FIND;
    if ((acts[i].op >= AGX_A_REGISTER && acts[i].op <= AGX_A_ROUTE) || (acts[i].op >= AGX_A_PUBLISH && acts[i].op <= AGX_A_FIND)) {
      uses_recep = true;
      rc_keys_used = std::max<uint32_t>(rc_keys_used, acts[i].pad1 + 1u);
    }
    uses_recep |= acts[i].op == AGX_A_TELL && (acts[i].pad0 & AGX_ROUTE_KEEP_SENDER) != 0;
  }
  // the apply kernels reserve kmax tell slots per message (single pass: the tell overwrites the
  // message's own consumed LDS slot; otherwise a bucket's tells live in [lo*kmax, (lo+cnt)*kmax)):
  // a case that tells more often would overwrite unprocessed mail or the next bucket's tells
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t tells = 0;
    for (uint32_t i = cases[c].act_first; i < (uint32_t)cases[c].act_first + cases[c].act_count; ++i)
      tells += acts[i].op == AGX_A_TELL || acts[i].op == AGX_A_ASK_SEND;  // (an ask's request takes the tell slot)
    if (tells > e->kmax)
      return set_err(AGX_EINVAL, "compiled behaviours: case %u tells %u times per message, max_emit is %u", c, tells,
                     e->kmax);
  }
  AGX_TRY(ensure_dev(e));
  hipFree(e->d_bcase);
  hipFree(e->d_bact);
  hipFree(e->d_bfirst);
  e->d_bcase = nullptr;
  e->d_bact = nullptr;
  e->d_bfirst = nullptr;
  AGX_TRY(dalloc(&e->d_bcase, std::max<uint32_t>(n_cases, 1)));
  AGX_TRY(dalloc(&e->d_bact, std::max<uint32_t>(n_acts, 1)));
  AGX_TRY(dalloc(&e->d_bfirst, n_beh + 1));
  if (n_cases) AGX_TRY(copy_sync(e, e->d_bcase, cases, n_cases * sizeof(agx_case), hipMemcpyHostToDevice));
  if (n_acts) AGX_TRY(copy_sync(e, e->d_bact, acts, n_acts * sizeof(agx_act), hipMemcpyHostToDevice));
  AGX_TRY(copy_sync(e, e->d_bfirst, first, (n_beh + 1) * 4ull, hipMemcpyHostToDevice));
  e->n_beh = n_beh;
  e->beh_stash = false;
  e->beh_fail = e->beh_svsig = e->beh_vstash = false;  // (checked against agx_set_supervision at agx_run)
  for (uint32_t c = 0; c < n_cases; ++c) {
    const uint32_t r = cases[c].result & ~AGX_CASE_SIGNAL;
    e->beh_stash |= r == AGX_RES_STASH || r == AGX_RES_UNSTASH_ALL;
    e->beh_fail |= r == AGX_RES_FAIL;
    e->beh_svsig |= sv_signal(cases[c]);
    e->beh_vstash |= cases[c].src1 == AGX_V_STASH || cases[c].src2 == AGX_V_STASH || cases[c].src3 == AGX_V_STASH ||
                     cases[c].src4 == AGX_V_STASH;
  }
  for (uint32_t i = 0; i < n_acts; ++i) e->beh_vstash |= acts[i].src == AGX_V_STASH || acts[i].dsrc == AGX_V_STASH;
  // supervision: a failing or stopping case's tells and a PreRestart / PostStop case's tells share the message's slots
  e->beh_sv_tells = 0;
  for (uint32_t b = 0; b < n_beh; ++b) {
    uint32_t fs = 0, sg = 0;
    for (uint32_t c = first[b]; c < first[b + 1]; ++c) {
      uint32_t tells = 0;
      for (uint32_t i = cases[c].act_first; i < (uint32_t)cases[c].act_first + cases[c].act_count; ++i)
        tells += acts[i].op == AGX_A_TELL;
      const uint32_t r = cases[c].result & ~AGX_CASE_SIGNAL;
      if (sv_signal(cases[c])) sg = std::max(sg, tells);
      else if (r == AGX_RES_FAIL || r == AGX_RES_STOPPED) fs = std::max(fs, tells);
    }
    e->beh_sv_tells = std::max(e->beh_sv_tells, fs + sg);
  }
  e->beh_ask_keys = 0;  // (checked against agx_set_ask and the key count at agx_run)
  e->beh_ask_unpaired = -1;
  for (uint32_t c = 0; c < n_cases; ++c)
    for (uint32_t i = cases[c].act_first; i < (uint32_t)cases[c].act_first + cases[c].act_count; ++i) {
      const agx_act& A = acts[i];
      if (A.op != AGX_A_ASK_ARM && A.op != AGX_A_ASK_SEND) continue;
      e->beh_ask_keys = std::max<uint32_t>(e->beh_ask_keys, A.word + 1u);
      // (within the case: ARM then the SEND of its key)
      const bool paired = A.op == AGX_A_ASK_ARM
                              ? i + 1u < (uint32_t)cases[c].act_first + cases[c].act_count && acts[i + 1].op == AGX_A_ASK_SEND &&
                                    acts[i + 1].word == A.word
                              : i > cases[c].act_first && acts[i - 1].op == AGX_A_ASK_ARM && acts[i - 1].word == A.word;
      if (!paired && e->beh_ask_unpaired < 0) e->beh_ask_unpaired = (int64_t)i;
    }
  e->beh_rt = false;  // (checked against agx_set_receive_timeout at agx_run)
  for (uint32_t i = 0; i < n_acts; ++i)
    e->beh_rt |= acts[i].op == AGX_A_SET_RECEIVE_TIMEOUT || acts[i].op == AGX_A_CANCEL_RECEIVE_TIMEOUT;
  e->beh_rt_tag = rt_tag;
  e->beh_passivate = false;  // (checked against agx_set_sharding at agx_run)
  for (uint32_t i = 0; i < n_acts; ++i) e->beh_passivate |= acts[i].op == AGX_A_PASSIVATE;
  e->beh_recep = uses_recep;  // (checked against agx_set_receptionist at agx_run)
  e->beh_rc_keys = rc_keys_used;
  e->beh_publish = uses_publish;  // (checked against agx_set_topics at agx_run)
  e->beh_listing = uses_listing;  // (checked against agx_set_listings at agx_run)
  e->beh_router = false;  // a hashed or random route (checked against agx_set_router_logics at agx_run)
  e->beh_hashed_keys = 0;
  e->beh_route_two = -1;
  for (uint32_t i = 0; i < n_acts; ++i) {
    if (acts[i].op != AGX_A_ROUTE) continue;
    const uint32_t sel = acts[i].pad0 & (AGX_ROUTE_BY_INDEX | AGX_ROUTE_HASHED | AGX_ROUTE_RANDOM);
    if ((sel & (sel - 1u)) && e->beh_route_two < 0) e->beh_route_two = i;
    e->beh_router |= (sel & (AGX_ROUTE_HASHED | AGX_ROUTE_RANDOM)) != 0;
    if (sel & AGX_ROUTE_HASHED) e->beh_hashed_keys |= 1u << (acts[i].pad1 & 7u);
  }
  e->beh_child = uses_child;  // (checked against agx_set_children at agx_run)
  e->beh_ctl_tags = ctl_tags;
  e->beh_watch = false;  // a watch action or a signal case (checked against agx_set_death_watch at agx_run)
  for (uint32_t c = 0; c < n_cases; ++c) e->beh_watch |= (cases[c].result & AGX_CASE_SIGNAL) != 0 && !sv_signal(cases[c]);
  for (uint32_t i = 0; i < n_acts; ++i) e->beh_watch |= acts[i].op >= AGX_A_WATCH && acts[i].op <= AGX_A_UNWATCH;
  e->beh_tm_keys = 0;  // the timer keys the tables use (checked against agx_set_timers at agx_run)
  auto tm_use = [&](uint32_t src, uint32_t word) {
    if (src == AGX_V_TIMER) e->beh_tm_keys = std::max(e->beh_tm_keys, word + 1u);
  };
  for (uint32_t c = 0; c < n_cases; ++c) {
    tm_use(cases[c].src1, cases[c].word1);
    tm_use(cases[c].src2, cases[c].word2);
    tm_use(cases[c].src3, cases[c].word3);
    tm_use(cases[c].src4, cases[c].word4);
  }
  for (uint32_t i = 0; i < n_acts; ++i) {
    tm_use(acts[i].src, acts[i].sword);
    tm_use(acts[i].dsrc, acts[i].dword);
    if (acts[i].op == AGX_A_TIMER_CANCEL_ALL) e->beh_tm_keys = std::max(e->beh_tm_keys, 1u);
    else if (acts[i].op >= AGX_A_TIMER_SINGLE && acts[i].op <= AGX_A_TIMER_CANCEL) e->beh_tm_keys = std::max<uint32_t>(e->beh_tm_keys, acts[i].word + 1u);
    // (an ask's key is checked apart: beh_ask_keys)
  }
  drop_graphs(e);  // the tables are kernel parameters captured in the superstep graphs
  return AGX_OK;
}

agx_status agx_set_delta_crdt(agx_engine* e, uint32_t max_delta_size) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (max_delta_size > AGX_DELTA_MAX_SIZE)
    return set_err(AGX_EINVAL, "max_delta_size %u > %u (DeltaPropagation rows are sized for it)", max_delta_size,
                   AGX_DELTA_MAX_SIZE);
  if (max_delta_size && e->kmax < 4) return set_err(AGX_EINVAL, "delta-CRDT replicas need max_emit >= 4");
  if (max_delta_size && e->n_global >= (1ull << 30)) return set_err(AGX_EINVAL, "delta-CRDT needs n_actors < 2^30");
  if (e->started && max_delta_size != e->delta_max) return set_err(AGX_ESTATE, "set delta-CRDT mode before agx_run");
  if (max_delta_size && (e->kinds_mask & kb(AGX_KIND_LWWMAP)))
    return set_err(AGX_EINVAL, "delta-CRDT replication on an engine with LWWMap replicas: they gossip their full state "
                   "(ORMap delta ops are left out)");
  if (max_delta_size && (e->kinds_mask & kb(AGX_KIND_ORMULTIMAP)))
    return set_err(AGX_EINVAL, "delta-CRDT replication on an engine with ORMultiMap replicas: they gossip their full "
                   "state (ORMap delta ops are left out)");
  if (max_delta_size && (e->kinds_mask & kb(AGX_KIND_PNCOUNTERMAP)))
    return set_err(AGX_EINVAL, "delta-CRDT replication on an engine with PNCounterMap replicas: they gossip their full "
                   "state (ORMap delta ops are left out)");
  e->delta_max = max_delta_size;
  for (uint32_t k = AGX_KIND_GCOUNTER; k <= AGX_KIND_ORSET; ++k)
    if (e->kinds_mask & kb(k)) AGX_TRY(enable_crdt(e, k));
  drop_graphs(e);
  return AGX_OK;
}

agx_status agx_set_lwwmap(agx_engine* e, uint32_t clock, uint64_t base) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (!(e->kinds_mask & kb(AGX_KIND_LWWMAP)))
    return set_err(AGX_EINVAL, "agx_set_lwwmap: the engine has no LWWMap replicas (register them first)");
  if (clock != AGX_LWW_CLOCK_DEFAULT && clock != AGX_LWW_CLOCK_REVERSE)
    return set_err(AGX_EINVAL, "agx_set_lwwmap: unknown clock %u (AGX_LWW_CLOCK_DEFAULT, AGX_LWW_CLOCK_REVERSE)", clock);
  if (base >= (1ull << 62)) return set_err(AGX_EINVAL, "agx_set_lwwmap: base must be < 2^62");
  if (e->started) return set_err(AGX_ESTATE, "set the LWWMap clock before the first agx_run");
  e->lww_clock = clock;
  e->lww_base = base;
  drop_graphs(e);  // (kernel arguments of the captured supersteps)
  return AGX_OK;
}

agx_status agx_set_lwwmap_delta(agx_engine* e, uint32_t max_delta_size) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  // (first: a multi-rank engine cannot register LWWMap replicas at all)
  if (e->R > 1) return set_err(AGX_EINVAL, "agx_set_lwwmap_delta: LWWMap replicas need a single-rank engine (n_ranks %u)", e->R);
  if (!(e->kinds_mask & kb(AGX_KIND_LWWMAP)))
    return set_err(AGX_EINVAL, "agx_set_lwwmap_delta: the engine has no LWWMap replicas (register them first)");
  if (max_delta_size == 0 || max_delta_size > AGX_DELTA_MAX_SIZE)
    return set_err(AGX_EINVAL, "agx_set_lwwmap_delta: max_delta_size %u is not in 1..%u (DeltaPropagation rows are sized for it)",
                   max_delta_size, AGX_DELTA_MAX_SIZE);
  if (e->kmax < 4) return set_err(AGX_EINVAL, "agx_set_lwwmap_delta: delta-CRDT replicas need max_emit >= 4");
  if (e->W < AGX_LWWMAP_DELTA_WORDS)
    return set_err(AGX_EINVAL, "agx_set_lwwmap_delta: LWWMap delta replication needs n_words >= %u (got %u)",
                   AGX_LWWMAP_DELTA_WORDS, e->W);
  if (e->started) return set_err(AGX_ESTATE, "set LWWMap delta replication before the first agx_run");
  // the row pitch of the mode: full-state rows carry the deltaVersions behind their data, and both row forms
  // stay below the length word of a DeltaPropagation (agx_lwwmap_delta.h kLdPitch)
  static_assert(kLdPitch % kRowAlign == 0 && kLdPitch > (2 * AGX_LWWMAP_WORDS + kRowAlign - 1) / kRowAlign * kRowAlign,
                "the row pitch of LWWMap delta replication is wider than the full-state engine's");
  if (e->pw < kLdPitch) {
    uint32_t* heap = nullptr;  // (the new heap first: a failed allocation leaves the engine as it was)
    AGX_TRY(dalloc_rows(&heap, 2 * e->heap_rows * kLdPitch));
    hipFree(e->d_heap);
    e->d_heap = heap;
    e->pw = kLdPitch;
  }
  e->lww_delta_max = max_delta_size;
  drop_graphs(e);  // (the apply variant and the row pitch are captured in the superstep graphs)
  return AGX_OK;
}

agx_status agx_set_ring(agx_engine* e, uint32_t stride) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  e->ring_stride = stride;
  drop_graphs(e);
  return AGX_OK;
}

agx_status agx_set_fanout(agx_engine* e, uint32_t k, uint64_t seed, const uint32_t* cdf, const uint32_t* perm,
                          uint64_t n) {
  if (!e || !cdf || !perm || n == 0) return set_err(AGX_EINVAL, "bad fanout args");
  if (k > e->kmax) return set_err(AGX_EINVAL, "fanout k=%u exceeds max_emit=%u", k, e->kmax);
  for (uint64_t i = 0; i < n; ++i)
    if (perm[i] >= e->n_global) return set_err(AGX_EINVAL, "perm entry out of range");
  AGX_TRY(ensure_dev(e));
  if (n >= (1ull << 32)) return set_err(AGX_EINVAL, "fanout table too large");
  for (uint64_t i = 1; i < n; ++i)
    if (cdf[i] < cdf[i - 1]) return set_err(AGX_EINVAL, "fanout cdf not monotone at %llu", (unsigned long long)i);
  // range index (zipf_dest): zidx[t] = first i with cdf[i] >= t << (32 - kZipfBits), clamped to n - 1,
  // zidx[Z] = n - 1; entry t = {perm[i], kZipfDirect} when zidx[t] == zidx[t + 1] = i (every u of the
  // range answers i), else the search range {zidx[t], zidx[t + 1]}
  const uint64_t Z = 1ull << kZipfBits;
  std::vector<uint32_t> zidx(Z + 1);
  for (uint64_t t = 0, i = 0; t < Z; ++t) {
    const uint64_t u = t << (32 - kZipfBits);
    while (i < n && cdf[i] < u) ++i;
    zidx[t] = (uint32_t)std::min<uint64_t>(i, n - 1);
  }
  zidx[Z] = (uint32_t)(n - 1);
  std::vector<uint2> zent(Z);
  for (uint64_t t = 0; t < Z; ++t)
    zent[t] = zidx[t] == zidx[t + 1] ? make_uint2(perm[zidx[t]], kZipfDirect) : make_uint2(zidx[t], zidx[t + 1]);
  hipFree(e->d_zcdf);
  hipFree(e->d_zperm);
  hipFree(e->d_zent);
  e->d_zcdf = e->d_zperm = nullptr;
  e->d_zent = nullptr;
  AGX_TRY(dalloc(&e->d_zcdf, n));
  AGX_TRY(dalloc(&e->d_zperm, n));
  AGX_TRY(dalloc(&e->d_zent, Z));
  AGX_TRY(copy_sync(e, e->d_zent, zent.data(), Z * sizeof(uint2), hipMemcpyHostToDevice));
  AGX_TRY(copy_sync(e, e->d_zcdf, cdf, n * 4, hipMemcpyHostToDevice));
  AGX_TRY(copy_sync(e, e->d_zperm, perm, n * 4, hipMemcpyHostToDevice));
  e->fan_k = k;
  e->fan_seed = seed;
  e->zipf_n = n;
  drop_graphs(e);
  return AGX_OK;
}

agx_status agx_set_graph(agx_engine* e, const uint64_t* row_ptr, const uint32_t* col) {
  if (!e || !row_ptr) return set_err(AGX_EINVAL, "bad graph args");
  // the whole row_ptr is checked before col is read: then col[0, row_ptr[n_actors]) is every index
  // read below, the length a binding checks its array against (agx_jni.c setGraph)
  for (uint64_t id = 0; id < e->n_global; ++id)
    if (row_ptr[id + 1] < row_ptr[id]) return set_err(AGX_EINVAL, "row_ptr not monotone at %llu", (unsigned long long)id);
  if (row_ptr[e->n_global] > row_ptr[0] && !col) return set_err(AGX_EINVAL, "bad graph args: null col");
  AGX_TRY(ensure_dev(e));
  // keep only the rows of local actors (rows indexed by local id)
  std::vector<uint64_t> row(e->n_local + 1, 0);
  std::vector<uint32_t> c;
  for (uint64_t l = 0; l < e->n_local; ++l) {
    uint64_t id = e->R > 1 ? e->h_gid[l] : l;
    uint64_t b = row_ptr[id], en = row_ptr[id + 1];
    for (uint64_t j = b; j < en; ++j) c.push_back(col[j]);
    row[l + 1] = c.size();
  }
  hipFree(e->d_row);
  hipFree(e->d_col);
  e->d_row = nullptr;
  e->d_col = nullptr;
  AGX_TRY(dalloc(&e->d_row, row.size()));
  AGX_TRY(dalloc(&e->d_col, c.size()));
  AGX_TRY(copy_sync(e, e->d_row, row.data(), row.size() * 8, hipMemcpyHostToDevice));
  if (!c.empty()) AGX_TRY(copy_sync(e, e->d_col, c.data(), c.size() * 4, hipMemcpyHostToDevice));
  e->graph_set = true;
  drop_graphs(e);
  return AGX_OK;
}

agx_status agx_set_graph_rmat(agx_engine* e, const uint64_t* row_ptr, uint32_t bits, uint32_t ta, uint32_t tb,
                              uint32_t tc, uint64_t seed) {
  if (!e || !row_ptr || bits == 0 || bits > 40) return set_err(AGX_EINVAL, "bad rmat graph args");
  AGX_TRY(ensure_dev(e));
  std::vector<uint64_t> lrow(e->n_local + 1, 0), gstart(std::max<uint64_t>(e->n_local, 1), 0);
  for (uint64_t l = 0; l < e->n_local; ++l) {
    const uint64_t id = e->R > 1 ? e->h_gid[l] : l;
    const uint64_t b = row_ptr[id], en = row_ptr[id + 1];
    if (en < b) return set_err(AGX_EINVAL, "row_ptr not monotone at %llu", (unsigned long long)id);
    gstart[l] = b;
    lrow[l + 1] = lrow[l] + (en - b);
  }
  hipFree(e->d_row);
  hipFree(e->d_col);
  e->d_row = nullptr;
  e->d_col = nullptr;
  uint64_t* d_gs = nullptr;
  AGX_TRY(dalloc(&e->d_row, lrow.size()));
  AGX_TRY(dalloc(&e->d_col, lrow.back()));
  AGX_TRY(dalloc(&d_gs, gstart.size()));
  AGX_TRY(copy_sync(e, e->d_row, lrow.data(), lrow.size() * 8, hipMemcpyHostToDevice));
  AGX_TRY(copy_sync(e, d_gs, gstart.data(), gstart.size() * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gen_rmat, dim3(grid_for(e->n_local / kThreads + 1, 8192)), dim3(kThreads), 0, e->stream,
                     e->d_row, d_gs, e->d_col, (uint32_t)e->n_local, bits, ta, tb, tc, seed, (uint32_t)e->n_global);
  hipError_t le = hipGetLastError();
  hipError_t se = hipStreamSynchronize(e->stream);
  hipFree(d_gs);
  if (le != hipSuccess || se != hipSuccess) return set_err(AGX_EDEVICE, "rmat generation failed");
  e->graph_set = true;
  drop_graphs(e);
  return AGX_OK;
}

// Host tells.  All or nothing: the tells are validated and counted before any is staged, so an
// AGX_EINVAL or AGX_ECAPACITY leaves the engine exactly as it was (no tell staged, no counter moved).
// Capacity: the messages in flight after staging -- the device's backlog and undelivered tells, the
// staged tells not yet consumed, and these -- must fit msg_capacity, or the first superstep's inbox
// would overflow its arenas.
agx_status in_flight_now(agx_engine* e, uint64_t* out);
agx_status agx_stage_tells(agx_engine* e, const uint32_t* dst, const uint32_t* src, const uint32_t* payload, size_t n) {
  if (!e || (n && (!dst || !payload))) return set_err(AGX_EINVAL, "bad tells");
  uint64_t take = 0;  // tells this rank stages (unknown refs are dead letters, other ranks' tells ignored)
  for (size_t i = 0; i < n; ++i) {
    const uint32_t d = dst[i];
    if (d >= e->n_global || (e->R > 1 && (e->h_route[d] >> kOwnerShift) != e->rank)) continue;
    const uint32_t sv = src ? src[i] : AGX_NO_SENDER;
    if ((sv & AGX_WIDE_BIT) && sv != AGX_NO_SENDER)
      return set_err(AGX_EINVAL, "tell %zu: sender %u is not an actor id (bit 31 tags CRDT state gossips)", i, sv);
    if (e->tm_keys && (payload[i] >> 24) == AGX_TAG_TIMER)
      return set_err(AGX_EINVAL, "tell %zu: message tag 0xFF is reserved for timer messages on an engine with timers", i);
    if (e->rt_on && (payload[i] >> 24) == AGX_TAG_RECEIVE_TIMEOUT)
      return set_err(AGX_EINVAL, "tell %zu: message tag 0xFB is reserved for receive-timeout envelopes on an engine with "
                     "receive timeouts", i);
    if (e->wd_slots && (payload[i] >> 24) == AGX_TAG_WATCH)
      return set_err(AGX_EINVAL, "tell %zu: message tag 0xFE is reserved for Terminated envelopes on an engine with death watch", i);
    if (e->d_child && ((payload[i] >> 24) == AGX_TAG_CREATE || (payload[i] >> 24) == AGX_TAG_STOP))
      return set_err(AGX_EINVAL, "tell %zu: message tags 0xFD and 0xFC are reserved for Create and Stop envelopes on an engine "
                     "with children", i);
    ++take;
  }
  if (take) {
    uint64_t infl = 0;
    AGX_TRY(in_flight_now(e, &infl));
    if (infl + take > e->cap)
      return set_err(AGX_ECAPACITY, "%llu staged tells do not fit: %llu messages in flight, msg_capacity %llu "
                     "(nothing staged)", (unsigned long long)take, (unsigned long long)infl, (unsigned long long)e->cap);
  }
  for (size_t i = 0; i < n; ++i) {
    const uint32_t d = dst[i];
    if (d >= e->n_global) {  // unknown ref -> deadLetters (counted once, on rank 0)
      if (e->rank == 0) { e->staged_total++; e->staged_dead++; }
      continue;
    }
    uint32_t key = d;
    if (e->R > 1) {
      uint32_t r = e->h_route[d];
      if ((r >> kOwnerShift) != e->rank) continue;
      key = r;
    }
    e->staged_total++;
    e->hs_key.push_back(key);
    e->hs_src.push_back(src ? src[i] : AGX_NO_SENDER);
    e->hs_pay.push_back(payload[i]);
  }
  return AGX_OK;
}

// Messages in flight on this rank right now (what agx_stats.in_flight would report): the device's
// backlog, undelivered tells and consumed-later staged chunks (one counter read-back, only once the
// engine has run), plus the host-staged tells not yet uploaded.
agx_status in_flight_now(agx_engine* e, uint64_t* out) {
  uint64_t dev = 0;
  if (e->started) {
    if (e->inflight_known) {
      dev = e->inflight_dev;
    } else {
      uint64_t s[kStatBlk];
      AGX_TRY(read_counters(e, s));
      dev = s[kStatInfl];
      e->inflight_dev = dev;
      e->inflight_known = true;  // (valid until the next agx_run)
    }
  }
  *out = dev + e->n_staged_dev + e->hs_key.size();
  return AGX_OK;
}

// The lock-free tell path: take the published tells (producer by producer, each in its order) into
// the host staging, exactly as agx_stage_tells would stage them -- but only as many as fit the
// message capacity.  The rest stay in the producers' queues (none is refused or lost: the
// reference's unbounded MPSC queue never refuses, AbstractNodeQueue.java:79-82) and
// agx_pump_idle reschedules the pump while any remain, so a burst larger than msg_capacity enters
// over several pumps as the engine drains (back-pressure across pumps).
agx_status take_tells(agx_engine* e) {
  if (!e->tq.pending()) return AGX_OK;
  uint64_t infl = 0;
  AGX_TRY(in_flight_now(e, &infl));
  uint64_t room = e->cap > infl ? e->cap - infl : 0;
  e->tq.take_while([&](uint32_t d, uint32_t s, uint32_t p) {
    const bool local = d < e->n_global && (e->R == 1 || (e->h_route[d] >> kOwnerShift) == e->rank);
    if (local) {
      if (!room) return false;  // stays queued for the next pump
      --room;
    }
    // (agx_tell rejected wide senders already; unknown refs and other ranks' tells take no room)
    const agx_status r = agx_stage_tells(e, &d, &s, &p, 1);
    (void)r;
    return true;
  });
  return AGX_OK;
}

agx_status agx_tell(agx_engine* e, uint32_t dst, uint32_t src, uint32_t payload, int32_t* schedule) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if ((src & AGX_WIDE_BIT) && src != AGX_NO_SENDER)
    return set_err(AGX_EINVAL, "tell: sender %u is not an actor id (bit 31 tags CRDT state gossips)", src);
  if (e->tm_keys && (payload >> 24) == AGX_TAG_TIMER)
    return set_err(AGX_EINVAL, "tell: message tag 0xFF is reserved for timer messages on an engine with timers");
  if (e->rt_on && (payload >> 24) == AGX_TAG_RECEIVE_TIMEOUT)
    return set_err(AGX_EINVAL, "tell: message tag 0xFB is reserved for receive-timeout envelopes on an engine with receive "
                   "timeouts");
  if (e->wd_slots && (payload >> 24) == AGX_TAG_WATCH)
    return set_err(AGX_EINVAL, "tell: message tag 0xFE is reserved for Terminated envelopes on an engine with death watch");
  if (e->d_child && ((payload >> 24) == AGX_TAG_CREATE || (payload >> 24) == AGX_TAG_STOP))
    return set_err(AGX_EINVAL, "tell: message tags 0xFD and 0xFC are reserved for Create and Stop envelopes on an engine with "
                   "children");
  const bool sched = e->tq.tell(dst, src, payload);
  if (schedule) *schedule = sched ? 1 : 0;
  return AGX_OK;
}

// The pump's last call (Mailbox.run's finally, Mailbox.scala:227-240: setAsIdle, then
// registerForExecution if the mailbox still has messages).  "Still has messages" is, here, either
// tells published but not taken (the queue re-check after the idle store) or mail in flight on the
// device after a run that stopped at its superstep budget (gpu.supersteps-per-pump) -- then the
// engine stays scheduled and the pump is submitted again.  After a failed run only the queue
// re-check applies (a broken engine must not spin its pump).
agx_status agx_pump_idle(agx_engine* e, int32_t* reschedule) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  bool again = false;
  if (e->last_run_ok && e->started) {
    uint64_t infl = 0;
    AGX_TRY(in_flight_now(e, &infl));
    again = infl > 0;  // (status stays "scheduled": this pump hands over to the next)
    if (!again && e->d_timers) {  // a pending timer keeps the engine scheduled
      std::vector<uint32_t> h;
      AGX_TRY(read_timer_head(e, h));
      for (uint32_t b = 0; b < e->nb; ++b) again |= h[kTmBucketOff + b] != kTmNone;
    }
    if (!again && e->d_watch) {  // a due slot, or a stop that watching slots have yet to see, keeps the engine scheduled
      AGX_TRY(flush_watch_starts(e));
      std::vector<uint32_t> h;
      AGX_TRY(read_watch_head(e, h));
      const uint32_t clk = h[kWdBucketOff + 2ull * e->nb];
      again = h[kWdStopW + (clk & 1u)] == clk && h[kWdAnyW + (clk & 1u)] == clk;
      for (uint32_t b = 0; b < e->nb; ++b) again |= h[kWdBucketOff + b] != 0u;
    }
  }
  if (!again) again = e->tq.pump_idle();
  if (reschedule) *reschedule = again ? 1 : 0;
  return AGX_OK;
}

agx_status agx_pump_cancel(agx_engine* e) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  e->tq.cancel_schedule();
  return AGX_OK;
}

agx_status agx_run(agx_engine* e, uint32_t max_supersteps, agx_stats* out) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  e->last_run_ok = false;
  AGX_TRY(ensure_dev(e));
  AGX_TRY(take_tells(e));
  e->inflight_known = false;  // (the supersteps below change the device's in-flight count)
  if (e->R > 1 && !e->comm) return set_err(AGX_ESTATE, "n_ranks > 1 needs agx_comm_init (or agx_group_run)");
  AGX_TRY(prepare_run(e));
  AGX_TRY(setup_rings(e));
  AGX_TRY(setup_ring_apply(e));
  AGX_TRY(setup_orset(e));
  e->started = true;
  if (e->R > 1) {
    AGX_TRY(run_multi_rccl(e, max_supersteps));
  } else {
    AGX_TRY(run_single(e, max_supersteps));
    AGX_TRY(timers_after_run(e));
    AGX_TRY(watch_after_run(e));
    AGX_TRY(super_after_run(e));
  }
  prof_collect(e);
  if (e->ident_on && getenv("AGX_IDENT_DEBUG")) {  // diagnostic: the last superstep's slice summaries
    const uint32_t nsl = (e->nb + kBlSlice - 1) / kBlSlice;
    std::vector<uint32_t> h((kMaxBlSlices + 1) * kSlSum), id(4);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(h.data(), e->d_slsum, h.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(id.data(), e->d_ident, 16, hipMemcpyDeviceToHost));
    fprintf(stderr, "[agx ident] on=%u rot=%u total=%u staged=%u |", id[0], id[1], id[2], h[kMaxBlSlices * kSlSum]);
    for (uint32_t i = 0; i < nsl; ++i)
      fprintf(stderr, " s%u{tot=%u fl=%u d=%u nd=%u pos=%u first=%u last=%u}", i, h[i * kSlSum], h[i * kSlSum + 1],
              h[i * kSlSum + 2], h[i * kSlSum + 3], h[i * kSlSum + 4], h[i * kSlSum + 5], h[i * kSlSum + 6]);
    fprintf(stderr, "\n");
  }
  if (e->d_dbg) {  // diagnostic: mean phase durations of k_bucket_apply blocks (last superstep)
    const uint64_t nbk = std::min<uint64_t>(e->nb, 4096);
    std::vector<unsigned long long> h(nbk * 16);
    HIP_TRY(hipMemcpy(h.data(), e->d_dbg, h.size() * 8, hipMemcpyDeviceToHost));
    double acc[8] = {0};
    unsigned long long t0min = ~0ull, t8max = 0;
    uint64_t nst = 0;  // blocks that recorded stamps (the skew launch runs fewer blocks)
    for (uint64_t b = 0; b < nbk; ++b) {
      if (!h[b * 16] || !h[b * 16 + 8]) continue;
      ++nst;
      for (int k = 0; k < 8; ++k) acc[k] += (double)(h[b * 16 + k + 1] - h[b * 16 + k]);
      t0min = std::min(t0min, h[b * 16]);
      t8max = std::max(t8max, h[b * 16 + 8]);
    }
    fprintf(stderr, "[agx stamps%s] mean cycles per phase over %llu blocks:", e->stamps_skew ? " (skew launch)" : "",
            (unsigned long long)nst);
    const char* nm[8] = {"range+alive", "sort", "->finish", "classify+backlog", "prefetch+phaseA", "scan", "phaseB", "hist+stats"};
    const char* nr[8] = {"count", "admission", "ring_heads", "placement", "prefetch", "drain", "tells", "words+hist"};
    for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.0f", (e->rg_on ? nr : nm)[k], nst ? acc[k] / nst : 0.0);
    fprintf(stderr, " | kernel span=%llu cycles\n", t8max - t0min);
    std::vector<std::pair<unsigned long long, uint64_t>> slow;
    for (uint64_t b = 0; b < nbk; ++b) slow.push_back({h[b * 16 + 10], b});
    std::sort(slow.rbegin(), slow.rend());
    fprintf(stderr, "[agx stamps] slowest buckets (cycles bucket inbox):");
    for (size_t i = 0; i < std::min<size_t>(6, slow.size()); ++i)
      fprintf(stderr, " %llu:%llu:%llu", slow[i].first, h[slow[i].second * 16 + 11], h[slow[i].second * 16 + 12]);
    fprintf(stderr, "\n");
    {  // device-clock (100 MHz) block start / end offsets within the launch (k_dense_fused only: slots 13 / 14)
      std::vector<double> st, en;
      unsigned long long s0 = ~0ull;
      for (uint64_t b = 0; b < nbk; ++b)
        if (h[b * 16 + 13] && h[b * 16 + 14]) s0 = std::min(s0, h[b * 16 + 13]);
      for (uint64_t b = 0; b < nbk; ++b)
        if (h[b * 16 + 13] && h[b * 16 + 14]) {
          st.push_back((h[b * 16 + 13] - s0) * 0.01);
          en.push_back((h[b * 16 + 14] - s0) * 0.01);
        }
      if (!st.empty()) {
        std::vector<double> du(st.size());
        for (size_t i = 0; i < st.size(); ++i) du[i] = en[i] - st[i];
        std::sort(st.begin(), st.end());
        std::sort(en.begin(), en.end());
        std::sort(du.begin(), du.end());
        auto q = [](const std::vector<double>& v, double f) { return v[std::min(v.size() - 1, (size_t)(f * v.size()))]; };
        fprintf(stderr, "[agx stamps] block start us (p0/p50/p90/max): %.2f %.2f %.2f %.2f | end: %.2f %.2f %.2f %.2f | "
                "duration: %.2f %.2f %.2f %.2f\n", q(st, 0), q(st, .5), q(st, .9), st.back(), q(en, 0), q(en, .5), q(en, .9),
                en.back(), q(du, 0), q(du, .5), q(du, .9), du.back());
      }
    }
    HIP_TRY(hipMemsetAsync(e->d_dbg, 0, h.size() * 8, e->stream));
  }
  // out == NULL: no counter read-back (one stream round trip less; agx_get_stats reads them
  // later), but the error word came back with the run's final sync
  const agx_status rs = out ? collect_stats(e, out, true) : error_status(e, e->h_stat[ST_ERROR]);
  e->last_run_ok = rs == AGX_OK;
  return rs;
}

agx_status agx_identity_supersteps(agx_engine* e, uint64_t* out) {
  if (!e || !out) return set_err(AGX_EINVAL, "bad identity_supersteps args");
  AGX_TRY(ensure_dev(e));
  uint64_t s[kStatBlk];
  AGX_TRY(read_counters(e, s));
  *out = s[ST_IDENT];
  return AGX_OK;
}

agx_status agx_ring_buckets(agx_engine* e, uint64_t* out) {
  if (!e || !out) return set_err(AGX_EINVAL, "bad ring_buckets args");
  AGX_TRY(ensure_dev(e));
  *out = 0;
  if (!e->ring_live) return AGX_OK;
  uint32_t n = 0;  // pool slots handed out (high-water mark: released slots are reused first)
  HIP_TRY(hipStreamSynchronize(e->stream));
  AGX_TRY(copy_sync(e, &n, e->d_ring_next, 4, hipMemcpyDeviceToHost));
  *out = std::min(n, e->ring_slots);
  return AGX_OK;
}

// agx_run with the run's device time on the engine stream: HIP events recorded before the first
// launch and after the last replay (single rank), so the host's own time around the run is not in it
agx_status agx_run_timed(agx_engine* e, uint32_t max_supersteps, agx_stats* out, float* device_ms) {
  if (!e || !device_ms) return set_err(AGX_EINVAL, "bad run_timed args");
  AGX_TRY(ensure_dev(e));
  for (auto& ev : e->tev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  HIP_TRY(hipEventRecord(e->tev[0], e->stream));
  e->timing = e->R == 1;
  e->tev1_recorded = false;
  const agx_status st = agx_run(e, max_supersteps, out);
  e->timing = false;
  if (st != AGX_OK) return st;
  // multi-rank, and a single-rank run that launched nothing through the replay loop (agx_run(0)
  // captures graphs and returns before it): the end event is recorded here, after the run's work
  if (!e->tev1_recorded) HIP_TRY(hipEventRecord(e->tev[1], e->stream));
  HIP_TRY(hipEventSynchronize(e->tev[1]));
  HIP_TRY(hipEventElapsedTime(device_ms, e->tev[0], e->tev[1]));
  return st;
}

agx_status agx_persist_info(agx_engine* e, uint64_t out[2]) {
  if (!e || !out) return set_err(AGX_EINVAL, "bad persist_info args");
  out[0] = e->persist_launches;
  out[1] = e->persist_supersteps;
  return AGX_OK;
}

agx_status agx_exchange_info(agx_engine* e, uint64_t out[6]) {
  if (!e || !out) return set_err(AGX_EINVAL, "bad exchange_info args");
  out[0] = e->mr_dev_steps;
  out[1] = e->mr_host_steps;
  out[2] = e->mr_sent_env;
  out[3] = e->mr_sent_rows;
  out[4] = e->mr_host ? 1u : 0u;
  out[5] = e->slab;
  return AGX_OK;
}

agx_status agx_get_stats(agx_engine* e, agx_stats* out) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  AGX_TRY(ensure_dev(e));
  return collect_stats(e, out, true);
}

agx_status agx_get_shape(agx_engine* e, uint64_t* n_actors, uint32_t* n_words) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (n_actors) *n_actors = e->n_global;
  if (n_words) *n_words = e->W;
  return AGX_OK;
}

agx_status agx_read_state(agx_engine* e, uint64_t first_id, uint64_t count, uint64_t* words, uint8_t* alive) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  if (first_id + count > e->n_global) return set_err(AGX_EINVAL, "range out of bounds");
  AGX_TRY(ensure_dev(e));
  AGX_TRY(sync_mirrors(e));
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t id = first_id + i, l;
    if (e->R > 1) {
      uint32_t r = e->h_route[id];
      if ((r >> kOwnerShift) != e->rank) continue;
      l = r & kLocalMask;
    } else {
      l = id;
    }
    if (words)
      for (uint32_t w = 0; w < e->W; ++w) words[i * e->W + w] = e->h_state[(uint64_t)w * e->n_local + l];
    if (alive) alive[i] = e->h_alive[l] & 1u;
  }
  return AGX_OK;
}

agx_status agx_comm_unique_id(uint8_t out[128]) {
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(out, &id, 128);
  return AGX_OK;
}

agx_status agx_comm_init(agx_engine* e, const uint8_t id[128]) {
  if (!e || !id) return set_err(AGX_EINVAL, "bad comm args");
  AGX_TRY(ensure_dev(e));
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  NCCL_TRY(ncclCommInitRank(&e->comm, (int)e->R, uid, (int)e->rank));
  return AGX_OK;
}

agx_status agx_group_run(agx_engine** engs, uint32_t n, uint32_t max_steps, agx_stats* out) {
  if (!engs || n == 0) return set_err(AGX_EINVAL, "bad group");
  if (n == 1) return agx_run(engs[0], max_steps, out);
  for (uint32_t i = 0; i < n; ++i) {
    if (!engs[i] || engs[i]->R != n || engs[i]->rank != i || engs[i]->n_global != engs[0]->n_global)
      return set_err(AGX_EINVAL, "group engines must be ranks 0..n-1 of one population");
    if (engs[i]->pw != engs[0]->pw || engs[i]->delta_max != engs[0]->delta_max || engs[i]->kmax != engs[0]->kmax ||
        engs[i]->W != engs[0]->W)
      return set_err(AGX_EINVAL, "group engines differ in row pitch / delta mode / max_emit / n_words");
    AGX_TRY(ensure_dev(engs[i]));
    AGX_TRY(prepare_run(engs[i]));
    AGX_TRY(setup_orset(engs[i]));
    engs[i]->started = true;
    engs[i]->inflight_known = false;
  }
  const uint32_t S = n + 2;
  std::vector<uint64_t> mat((size_t)n * S);
  std::vector<Plan> plans(n);
  for (uint32_t s = 0; s < max_steps; ++s) {
    for (uint32_t i = 0; i < n; ++i) AGX_TRY(phase1(engs[i]));
    for (uint32_t i = 0; i < n; ++i) {
      agx_engine* e = engs[i];
      HIP_TRY(hipMemcpyAsync(&mat[(size_t)i * S], e->d_cvec, S * 8, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
    uint64_t total = 0;
    for (auto v : mat) total += v;
    if (total == 0) break;
    for (uint32_t i = 0; i < n; ++i) {
      make_plan(engs[i], mat.data(), plans[i]);
      if (plans[i].n_bl + plans[i].n_recv + plans[i].n_staged > engs[i]->cap)
        return set_err(AGX_ECAPACITY, "rank %u over capacity", i);
    }
    // loopback exchange: receiver i pulls its slice of every sender's partitioned buffer
    for (uint32_t i = 0; i < n; ++i) {
      agx_engine* r = engs[i];
      for (uint32_t q = 0; q < n; ++q) {
        uint64_t cnt = plans[i].recv_cnt[q];
        if (!cnt) continue;
        agx_engine* snd = engs[q];
        uint64_t so = plans[q].send_off[i], ro = plans[i].recv_off[q];
        HIP_TRY(hipMemcpyAsync(r->A.key + ro, snd->s2.key + so, cnt * 4, hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(r->A.src + ro, snd->s2.src + so, cnt * 4, hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(r->A.pay + ro, snd->s2.pay + so, cnt * 4, hipMemcpyDeviceToDevice, r->stream));
        if (r->pw && q != i)
          HIP_TRY(hipMemcpyAsync(r->d_rx + ro * r->pw, snd->d_s2rows + so * snd->pw, cnt * r->pw * 4ull,
                                 hipMemcpyDeviceToDevice, r->stream));
      }
      AGX_TRY(fix_rx(r, plans[i]));
    }
    for (uint32_t i = 0; i < n; ++i) {
      Plan& p = plans[i];
      AGX_TRY(phase2(engs[i], p.n_bl + p.n_recv + p.n_staged, p.n_bl + p.n_recv));
    }
    for (uint32_t i = 0; i < n; ++i) HIP_TRY(hipStreamSynchronize(engs[i]->stream));
  }
  agx_stats tot{};
  for (uint32_t i = 0; i < n; ++i) {
    prof_collect(engs[i]);
    agx_stats st{};
    AGX_TRY(collect_stats(engs[i], &st, true));
    tot.delivered += st.delivered;
    tot.dead_letters += st.dead_letters;
    tot.unhandled += st.unhandled;
    tot.emitted += st.emitted;
    tot.staged += st.staged;
    tot.supersteps = std::max(tot.supersteps, st.supersteps);
    tot.in_flight += st.in_flight;
    tot.bytes_alg += st.bytes_alg;
  }
  if (out) *out = tot;
  return AGX_OK;
}

agx_status agx_mr_plan(const uint64_t* mat, uint32_t R, uint32_t rank, uint32_t slab, uint64_t cap, uint32_t* code,
                       uint64_t* send_off, uint64_t* recv_off, uint64_t* n_backlog) {
  if (!mat || !code || R == 0 || R > AGX_MAX_RANKS || rank >= R) return set_err(AGX_EINVAL, "bad mr_plan args");
  MrPlan p;
  mr_decide(mat, R, rank, slab, cap, p);
  *code = p.code;
  for (uint32_t q = 0; q <= R; ++q) {
    if (send_off) send_off[q] = p.soff[q];
    if (recv_off) recv_off[q] = p.roff[q];
  }
  if (n_backlog) *n_backlog = p.nbl;
  return AGX_OK;
}

agx_status agx_exchange_plan(const uint64_t* mat, uint32_t R, uint32_t rank, uint64_t* send_cnt, uint64_t* send_off,
                             uint64_t* recv_cnt, uint64_t* recv_off, uint64_t* inflight) {
  if (!mat || R == 0 || R > AGX_MAX_RANKS || rank >= R) return set_err(AGX_EINVAL, "bad plan args");
  agx_engine tmp;
  tmp.R = R;
  tmp.rank = rank;
  Plan p;
  make_plan(&tmp, mat, p);
  for (uint32_t q = 0; q < R; ++q) {
    if (send_cnt) send_cnt[q] = p.send_cnt[q];
    if (send_off) send_off[q] = p.send_off[q];
    if (recv_cnt) recv_cnt[q] = p.recv_cnt[q];
    if (recv_off) recv_off[q] = p.recv_off[q];
  }
  if (inflight) *inflight = p.total_inflight;
  return AGX_OK;
}

agx_status agx_profile_enable(agx_engine* e, int on) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  e->prof = on != 0;
  return AGX_OK;
}

agx_status agx_profile_reset(agx_engine* e) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  prof_collect(e);
  for (int i = 0; i < K_NCLASS; ++i) {
    e->prof_ms[i] = 0;
    e->prof_n[i] = 0;
    e->prof_items[i] = 0;
  }
  return AGX_OK;
}

agx_status agx_profile_read(agx_engine* e, char (*names)[32], double* total_ms, uint64_t* launches, uint64_t* items,
                            uint32_t cap, uint32_t* n) {
  if (!e) return set_err(AGX_EINVAL, "null engine");
  prof_collect(e);
  uint32_t k = 0;
  for (int i = 0; i < K_NCLASS && k < cap; ++i, ++k) {
    if (names) {
      strncpy(names[k], kClassNames[i], 31);
      names[k][31] = 0;
    }
    if (total_ms) total_ms[k] = e->prof_ms[i];
    if (launches) launches[k] = e->prof_n[i];
    if (items) items[k] = e->prof_items[i];
  }
  if (n) *n = K_NCLASS;
  return AGX_OK;
}

}  // extern "C"
