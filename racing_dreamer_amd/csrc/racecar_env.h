// What the units with entry points share of a handle (not part of the public interface): struct rc_env, the error and
// timing helpers, the arena layout.  racecar_abi.hip creates and destroys the handle; every other unit works on its fields.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#pragma GCC visibility push(default)       // the library exports the rc_* interface and nothing else (build.py: -fvisibility=hidden)
#include "../../include/racecar_hip.h"
#pragma GCC visibility pop
#include "racecar_internal.h"
#include "racecar_policy.h"
#include "racecar_episode.h"

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));      // sets rc_last_error(); returns `code` (racecar_abi.hip)


#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(RC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline uint32_t seed_lo(uint64_t seed) { return (uint32_t)(seed & 0xffffffffu); }      // the halves the kernels' Philox keys take
inline uint32_t seed_hi(uint64_t seed) { return (uint32_t)(seed >> 32); }

// bytes per car of every rc_field, in arena order
const size_t kFieldBytes[RC_F_COUNT] = {
    RC_N_BEAMS * 4, 24, 24, 4, 8, 4, 4, 4, 4, RC_PATCH * RC_PATCH,   // LIDAR .. OCCUPANCY
    4, 4, 4, 1, 1, 1, 1, 1, 1, 4, 4, 8,                               // PROGRESS .. ACTION_IN
};

struct Layout {
    size_t offset[RC_F_COUNT];
    size_t bytes[RC_F_COUNT];
    size_t slab_bytes;   // LIDAR..TIME (+OCCUPANCY when rendered)
    size_t total;
};

// The arena holds `n_cars` cars; a handle that owns only cars [first_car, first_car + n_own) of it (rc_config::arena_total_cars:
// several handles - one per track - fill ONE set of output arrays) gets the offsets and sizes of ITS slice of every section.
inline Layout make_layout(int n_cars, bool occupancy, int first_car = 0, int n_own = -1) {
    Layout l{};
    if (n_own < 0) n_own = n_cars;
    size_t off = 0;
    for (int f = 0; f < RC_F_COUNT; ++f) {
        size_t b = kFieldBytes[f] * (size_t)n_cars;
        if (f == RC_F_OCCUPANCY && !occupancy) b = 0;
        l.offset[f] = off + (b ? kFieldBytes[f] * (size_t)first_car : 0);
        l.bytes[f] = b ? kFieldBytes[f] * (size_t)n_own : 0;
        if (f == (occupancy ? RC_F_OCCUPANCY : RC_F_TIME)) l.slab_bytes = off + b;
        off = align_up(off + b, 64);
    }
    l.total = off;
    return l;
}

// The half-size trajectory record (rc_set_compact_slab): uint16 LiDAR rows, then a copy of the arena's POSE..TIME
// sections (same relative layout, 64-byte aligned sections).
struct CompactLayout {
    size_t lidar_bytes;      // n * 1080 * 2, rounded up to 64
    size_t summary_src_off;  // offset of RC_F_POSE in the arena
    size_t summary_bytes;    // RC_F_POSE .. end of RC_F_TIME
    size_t total;
};

inline CompactLayout make_compact(const Layout &l, int n_cars) {
    CompactLayout c{};
    c.lidar_bytes = align_up((size_t)n_cars * RC_N_BEAMS * 2, 64);
    c.summary_src_off = l.offset[RC_F_POSE];
    c.summary_bytes = l.offset[RC_F_TIME] + l.bytes[RC_F_TIME] - l.offset[RC_F_POSE];
    c.total = align_up(c.lidar_bytes + c.summary_bytes, 64);
    return c;
}

// Device tables of one compiled track (bitmaps, progress grid, spawn table, the scan's rectangle planes and first-trip
// table: 30 - 420 MB, built on the device in 20 - 100 ms).  They are read-only and depend on nothing but the track, so
// handles of one process that load the same track on the same device share one copy: the second rc_load_track of a
// track costs a hash of its inputs instead of an upload and a rebuild (tests and multi-handle clients create many).
struct TrackTables {
    int device = 0;
    void *mem = nullptr;
    // what the tables were built from, compared on a cache hit besides the 64-bit key: shape, geometry and a second,
    // independent checksum of the arrays (a key collision must not hand a handle another track's tables)
    int32_t h = 0, w = 0, pitch = 0, n_centerline = 0;
    float res = 0.f, ox = 0.f, oy = 0.f;
    uint64_t sum2 = 0;
    RcTrackDev t{};
    size_t lds_bytes = 0;
    RcLabTables lab{};       // scan variants 1-5: built by the lab library on first request (rc_set_raycast_variant, under the track
                             // mutex), shared by the handles of this track like `mem`, freed here - no call into the lab
    ~TrackTables() {
        if (mem || lab.free_blocks) (void)hipSetDevice(device);
        if (mem) (void)hipFree(mem);
        if (lab.free_blocks) (void)hipFree(const_cast<uint8_t *>(lab.free_blocks));
    }
};

struct EventPair {
    hipEvent_t a, b;
    int kernel;
};
// The episode log's launches of a step are timed like a kernel, under an accumulator of their own behind the public ones
// (rc_kernel_time does not know it: rc_episode_log_time reads it).
constexpr int kTimeEpisodeLog = RC_K_COUNT;
// ... and so is rc_look_ahead's launch (rc_look_ahead_time reads it)
constexpr int kTimeLookAhead = RC_K_COUNT + 1;
constexpr int kTimeCount = RC_K_COUNT + 2;

// A table of up to 8 RcParams on the device that follows its host-side contents in stream order (rc_step_group: one entry per
// handle; a track set: one per track).  A copy is queued only when an entry or the count changed since the last upload, from one
// of four pinned slots taken in turn, none rewritten before its copy has run.
static_assert(RC_GROUP_MAX == RC_TS_MAX, "one staged table type serves the group and the track set");
struct StagedTable {
    RcParams *dev = nullptr;
    RcParams *host = nullptr;      // [4][RC_GROUP_MAX], pinned
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t slot = 0;
    int n = 0;                     // entries of the last upload; 0: the next sync uploads
    RcParams last[RC_GROUP_MAX];
    int alloc() {                  // on first use (a failure half way is made up for by the next call)
        if (!dev) HIP_TRY(hipMalloc((void **)&dev, sizeof(RcParams) * RC_GROUP_MAX));
        if (!host) HIP_TRY(hipHostMalloc((void **)&host, sizeof(RcParams) * RC_GROUP_MAX * 4, hipHostMallocDefault));
        for (hipEvent_t &e : ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return RC_OK;
    }
    int sync(const RcParams *want, int n_want, hipStream_t stream) {
        if (n == n_want && std::memcmp(want, last, sizeof(RcParams) * n_want) == 0) return RC_OK;
        n = 0;
        const uint32_t k = slot++ & 3u;
        HIP_TRY(hipEventSynchronize(ev[k]));
        RcParams *stage = host + (size_t)k * RC_GROUP_MAX;
        std::memcpy(stage, want, sizeof(RcParams) * n_want);
        std::memcpy(last, want, sizeof(RcParams) * n_want);
        HIP_TRY(hipMemcpyAsync(dev, stage, sizeof(RcParams) * n_want, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ev[k], stream));
        n = n_want;
        return RC_OK;
    }
    void free() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

struct P2p;                        // the peer-copy all-gather's state (racecar_gather.hip)
struct RcFit;                      // the critic's, the reward head's and the actor's optimizers (racecar_fit.hip)
struct RcDreamGrad;                // the dream's backward pass: transposed weight images and the activation stash (racecar_dream_grad.hip)
struct RcReturnsGrad;              // the actor loss's backward pass: the same for the prior and the three heads (racecar_returns_grad.hip)

struct rc_env {
    rc_config cfg{};
    int n_cars = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // device memory
    void *arena = nullptr;
    bool own_arena = false;
    bool shared_arena = false;     // this handle fills a slice of a larger arena (rc_config::arena_total_cars)
    Layout layout{};
    void *state_mem = nullptr;
    std::shared_ptr<TrackTables> track;   // shared with the other handles that loaded the same track on this device
    uint8_t *mask_dev = nullptr;
    float *actions_in = nullptr;   // inside the arena the handle was created with (RC_F_ACTION_IN)
    void *out_arena = nullptr;     // where the output fields currently point (rc_set_arena)
    RcParams params{};
    RcLaunchInfo launch{};
    bool has_track = false;
    bool was_reset = false;
    // profiling
    uint32_t profiling = 0;        // bit k set: time kernel k with HIP events (the episode log's launches: any bit)
    std::vector<EventPair> pending;
    std::vector<EventPair> free_events;
    double k_ms[kTimeCount] = {0};         // (behind the public ones: kTimeEpisodeLog, kTimeLookAhead)
    uint64_t k_n[kTimeCount] = {0};
    int32_t dbg[RC_DBG_COUNT] = {0};   // rc_debug_set: experiment / validation knobs, all 0 = production behaviour
    // half-size record + multi-GPU gather
    CompactLayout compact{};
    void *compact_slab = nullptr;      // caller-owned device buffer of compact.total bytes, or null
    void *comm = nullptr;              // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_gathered = nullptr;
    bool gather_pending = false;
    P2p *p2p = nullptr;                // peer-copy all-gather (rc_p2p_setup), else null
    // obs_type lidar_occupancy_reference (racecar_patch_exact.h): the source frame (rc_set_source_frame), the spline
    // coefficients' scratch for one chunk of cars, Pillow's integer tables on the device
    RcExactParams exact{};
    bool has_frame = false;
    int exact_chunk = 0;
    void *exact_mem = nullptr;
    // rc_policy_load: the padded weights (one allocation), the agent's state [n_cars][232], the pointers into the weights
    float *pol_mem = nullptr;
    float *pol_state = nullptr;
    RcPolicyDev pol{};
    RcPolicySampleDev pol_s{};
    RcImagineDev pol_i{};              // rc_policy_imagine: img2 / img3 (in pol_mem, when rc_policy_load was given them) and the reward head
    float *pol_heads_mem = nullptr;    // rc_policy_load_heads
    RcDecodeDev pol_d{};               // rc_policy_decode: the decoder's repacked arrays (null = none loaded)
    float *pol_dec_mem = nullptr;      // rc_policy_load_decoder
    RcLidarDecodeDev pol_ld{};         // rc_policy_decode_lidar: the LiDAR distance decoder's images (null = none loaded)
    float *pol_ldec_mem = nullptr;     // rc_policy_load_lidar_decoder
    RcCriticDev pol_c{};               // rc_policy_returns: the value head and the pcont head (null = none loaded)
    float *pol_critic_mem = nullptr;   // rc_policy_load_critic
    RcFit *fit = nullptr;              // rc_policy_fit_begin: the heads' optimizers and their scratch (racecar_fit.hip)
    RcDreamGrad *dgrad = nullptr;      // rc_policy_dream_grad: made at its first call, dropped with the weights it was made from
    bool dgrad_reward_stale = false;   // a reward fit step moved the head under dgrad's two transposed images of it: the next call remakes them
    RcReturnsGrad *rgrad = nullptr;    // rc_policy_returns_grad: made at its first call, dropped with the weights it was made from
    uint32_t rgrad_stale = 0;          // RC_RGRAD_* bits: a fit step moved that head under rgrad's transposed images of it
    rc_policy_sampling pol_sampling{(uint32_t)sizeof(rc_policy_sampling), RC_POLICY_MODE_MEAN, 0u, 0.0f};      // rc_policy_set_sampling
    float *ftg_prev = nullptr;         // rc_follow_the_gap_reference: previous heading per car (NaN = none), allocated on first use
    float *vp_mem = nullptr;           // RcParams::vparams, [n_cars][RC_VP_COUNT] (nominal values while randomization is off)
    void *order_mem = nullptr;         // RcStateDev::order + the sort's bucket counters (batches of RC_ORDER_MIN_CARS cars and more)
    uint32_t order_age = 0;            // observations since the cars were last sorted by track position
    const float *last_scan_rows = nullptr;   // the LiDAR rows the last scan of this handle wrote (the small batches' cost keys)
    StagedTable group_table;           // rc_step_group (this handle as the first of a group): the blocks' RcParams as the last launch saw them
    // track set (rc_set_track_set): the source handles, the per-env arrays, the table of RcParams (one per track), the render's LDS bytes
    std::vector<rc_env *> ts_src;
    void *ts_mem = nullptr;            // track [num_envs] | next [num_envs] | list [n_cars] | start [RC_TS_MAX + 1] | counts, cursors
                                       // [2 RC_TS_MAX] | started [num_envs]
    StagedTable ts_table;
    size_t ts_patch_lds = 0;
    // episode log (rc_episode_log_enable): the running sums, counters, cursor and workgroup counts (one allocation), the rows,
    // the calls since enable / clear
    bool ep_on = false;
    void *ep_mem = nullptr;
    void *ep_rows = nullptr;
    uint64_t ep_calls = 0;
    RcEpisodeDev ep{};
};

int drain_events(rc_env *env);      // folds the finished event pairs into the accumulators (racecar_abi.hip)
int fit_release(rc_env *env);       // closes the critic's optimizers: whoever replaces or drops the critic (racecar_fit.hip)
int fit_release_reward(rc_env *env);      // closes the reward head's optimizer: whoever replaces or drops the reward head
int fit_release_actor(rc_env *env);       // closes the actor's optimizer: whoever replaces or drops the actor
int dream_grad_release(rc_env *env);      // drops the transposed images and the stash: whoever replaces or drops the prior or the reward head
int dream_grad_run(rc_env *env, RcDreamGradCall &c, int64_t chunk_rows);      // racecar_dream_grad.hip: the chunks of one rc_policy_dream_grad
enum { RC_RGRAD_REWARD = 1u, RC_RGRAD_VALUE = 2u, RC_RGRAD_PCONT = 4u };
int returns_grad_release(rc_env *env);    // drops the transposed images and the stash: whoever replaces or drops the prior, the reward head or the critic
int returns_grad_run(rc_env *env, RcReturnsGradCall &c, int64_t chunk_rows);  // racecar_returns_grad.hip: the chunks of one rc_policy_returns_grad

// Times what lies between begin() and end() under accumulator `kernel`.  One launch: the launch itself carries the two timestamps
// (rck_set_launch_events).  `bracket`: the pair is recorded on the stream around whatever is queued in between (the episode log's
// step is two dependent launches).
struct KernelTimer {
    rc_env *env;
    EventPair ep{};
    bool on = false, bracket = false;
    int begin(rc_env *e, int kernel, bool bracket_mode = false) {
        env = e;
        bracket = bracket_mode;
        if (kernel >= RC_K_COUNT ? e->profiling == 0 : !((e->profiling >> kernel) & 1u)) return RC_OK;
        if (e->pending.size() >= 4096) {
            int rc = drain_events(e);
            if (rc) return rc;
        }
        if (!e->free_events.empty()) {
            ep = e->free_events.back();
            e->free_events.pop_back();
        } else {
            HIP_TRY(hipEventCreate(&ep.a));
            HIP_TRY(hipEventCreate(&ep.b));
        }
        ep.kernel = kernel;
        if (bracket) HIP_TRY(hipEventRecord(ep.a, e->stream));
        else rck_set_launch_events(ep.a, ep.b);      // the launch that follows carries the two timestamps itself
        on = true;
        return RC_OK;
    }
    int end() {
        if (!on) return RC_OK;
        if (bracket) HIP_TRY(hipEventRecord(ep.b, env->stream));
        env->pending.push_back(ep);
        return RC_OK;
    }
};

#define TIMED(env, kernel, launch_expr)                 \
    do {                                                \
        KernelTimer _t;                                 \
        int _rc = _t.begin(env, kernel);                \
        if (_rc) return _rc;                            \
        HIP_TRY(launch_expr);                           \
        _rc = _t.end();                                 \
        if (_rc) return _rc;                            \
    } while (0)

// what racecar_abi.hip's reset, step and destroy call in the other units
void episode_bind(rc_env *env);     // racecar_episode.hip
int episode_step(rc_env *env);
void gather_release(rc_env *env);   // racecar_gather.hip: the peer-copy transport, the communicator and its stream
void policy_release(rc_env *env);   // racecar_policy.hip: the agent's weights and state, the prior's layers and the reward head
