// Rows out of recorded arenas and records between GPUs: the ring gather and the window sampler of a replay store
// (rc_gather_rows, rc_sample_*), the RCCL all-gather bound at run time (rc_comm_*, rc_gather_*) and the peer-copy
// all-gather over hipIpc (rc_p2p_*) - kernels, launchers, entry points.  Nothing here is on the step's path.
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <new>

#include "racecar_env.h"
#include "racecar_device.h"

typedef unsigned v4u __attribute__((ext_vector_type(4)));


// ---- rows out of a ring of arenas (rc_gather_rows: the window gather of replay.TrajectoryRing.sample) --------------------
// One wave per output row r: the record of car car_idx[r] in ring slot slot_idx[r], field by field, into the field's section
// of the output (row r of section f at out + sec[f] + r * bpc[f]).  The LiDAR row goes as 270 16-byte vectors, the small
// fields as words / bytes.
struct RcGatherRows {
    size_t src_off[RC_GATHER_MAX_FIELDS], dst_off[RC_GATHER_MAX_FIELDS];
    uint32_t bpc[RC_GATHER_MAX_FIELDS];
    int32_t n_fields;
    // rc_sample_batch (one launch for a whole training batch): fields of `obs_mask` (by position in this table) read
    // slot_obs_idx instead of slot_idx - a terminal row takes its observation from the record before it - and the first row
    // of a window that starts an episode (meta[4 w + 3]) gets `reset_word` in the fields of `reset_mask`: the reference's
    // reset row (action 0, reward 0, discount 1, time 0, progress -1: dreamer/wrappers.py:221-226).  length = 0: plain gather
    uint32_t obs_mask, reset_mask;
    uint32_t reset_word[RC_GATHER_MAX_FIELDS];
    const int32_t *slot_obs_idx, *meta;
    int32_t length;
};
__global__ __launch_bounds__(256) void rc_gather_rows_kernel(const char *__restrict__ ring, size_t slot_bytes, const int32_t *__restrict__ slot_idx,
                                                             const int32_t *__restrict__ car_idx, int n_rows, RcGatherRows g, char *__restrict__ out) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const unsigned lane = threadIdx.x & 63u;
    const size_t slot_plain = (size_t)slot_idx[row] * slot_bytes;
    const size_t slot_obs = g.length > 0 ? (size_t)g.slot_obs_idx[row] * slot_bytes : slot_plain;
    const size_t car = (size_t)car_idx[row];
    const bool reset_row = g.length > 0 && g.reset_mask != 0u && row % g.length == 0 && g.meta[4 * (row / g.length) + 3] != 0;
    for (int f = 0; f < g.n_fields; ++f) {
        const uint32_t n = g.bpc[f];
        const size_t slot = ((g.obs_mask >> f) & 1u) ? slot_obs : slot_plain;
        const char *src = ring + slot + g.src_off[f] + car * n;
        char *dst = out + g.dst_off[f] + (size_t)row * n;
        if (reset_row && ((g.reset_mask >> f) & 1u)) {          // (reset fields are 4 or 8 bytes of float32)
            for (uint32_t o = lane * 4u; o < n; o += 64u * 4u) *reinterpret_cast<uint32_t *>(dst + o) = g.reset_word[f];
            continue;
        }
        if ((n & 15u) == 0u) {                                   // (sections are 64-byte aligned and n is a multiple of 16: aligned vectors)
            for (uint32_t o = lane * 16u; o < n; o += 64u * 16u) *reinterpret_cast<v4u *>(dst + o) = *reinterpret_cast<const v4u *>(src + o);
        } else if ((n & 3u) == 0u) {
            for (uint32_t o = lane * 4u; o < n; o += 64u * 4u) *reinterpret_cast<uint32_t *>(dst + o) = *reinterpret_cast<const uint32_t *>(src + o);
        } else {
            for (uint32_t o = lane; o < n; o += 64u) dst[o] = src[o];
        }
    }
}

hipError_t rck_gather_rows(const void *ring, size_t slot_bytes, const int32_t *slot_idx, const int32_t *car_idx, int n_rows,
                           const size_t *src_off, const size_t *dst_off, const uint32_t *bpc, int n_fields, void *out, hipStream_t s,
                           const RcBatchRows *batch) {
    RcGatherRows g{};
    g.n_fields = n_fields;
    for (int f = 0; f < n_fields; ++f) { g.src_off[f] = src_off[f]; g.dst_off[f] = dst_off[f]; g.bpc[f] = bpc[f]; }
    if (batch != nullptr) {
        g.obs_mask = batch->obs_mask; g.reset_mask = batch->reset_mask; g.slot_obs_idx = batch->slot_obs_idx; g.meta = batch->meta;
        g.length = batch->length;
        for (int f = 0; f < n_fields; ++f) g.reset_word[f] = batch->reset_word[f];
    }
    hipLaunchKernelGGL(rc_gather_rows_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, (const char *)ring, slot_bytes, slot_idx, car_idx,
                       n_rows, g, (char *)out);
    return hipGetLastError();
}

// ---- window starts of a replay sampler (rc_sample_windows): one wave per window.  Draw (first record, car) - Philox keyed by
// the caller's seed, counter (window, try, draw) - until the `length` records of that car from ring age t0 on stay inside one
// episode: no fresh record strictly inside, a fresh LAST record only if it is the episode's terminal one (done, written by
// auto-reset).  Lanes test the records of the window side by side.  Then the window's rows for rc_gather_rows.
__global__ __launch_bounds__(256) void rc_sample_windows_kernel(RcSampleWindows a) {
    const int win = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (win >= a.n_windows) return;
    const int lane = threadIdx.x & 63;
    int t0 = 0, car = 0;
    bool ok = false;
    for (int attempt = 0; attempt < a.max_tries && !ok; ++attempt) {
        const rcd::u32x4 r = rcd::philox4x32((uint32_t)win, (uint32_t)attempt, a.draw, 0x57494e44u, a.seed_lo, a.seed_hi);
        t0 = (int)(r.x % (uint32_t)a.n_start);
        car = (int)(r.y % (uint32_t)a.n_cars);
        bool bad = false;
        for (int j = lane; j < a.length; j += 64) {
            if (j == 0) continue;
            const size_t slot = (size_t)((a.oldest + t0 + j) % a.capacity) * a.slot_bytes;
            const bool fresh = a.ring[slot + a.fresh_off + car] != 0;
            bad |= fresh && (j < a.length - 1 || a.ring[slot + a.done_off + car] == 0);
        }
        ok = __builtin_amdgcn_ballot_w64(bad) == 0ull;
    }
    if (!ok && lane == 0) atomicAdd(a.failed, 1u);
    const size_t last = (size_t)((a.oldest + t0 + a.length - 1) % a.capacity) * a.slot_bytes;
    const bool terminal = a.length > 1 && a.ring[last + a.fresh_off + car] != 0 && a.ring[last + a.done_off + car] != 0;
    for (int j = lane; j < a.length; j += 64) {
        const int slot = (a.oldest + t0 + j) % a.capacity;
        const size_t o = (size_t)win * a.length + j;
        a.slot_idx[o] = slot;
        // a terminal row takes its OBSERVATION from the record before it: the new episode's observation is not this episode's
        a.slot_obs_idx[o] = (terminal && j == a.length - 1) ? (a.oldest + t0 + j - 1) % a.capacity : slot;
        a.car_idx[o] = car;
    }
    if (lane == 0) {
        const size_t first = (size_t)((a.oldest + t0) % a.capacity) * a.slot_bytes;
        a.meta[4 * win] = t0; a.meta[4 * win + 1] = car; a.meta[4 * win + 2] = terminal ? 1 : 0;
        a.meta[4 * win + 3] = a.ring[first + a.fresh_off + car] != 0 ? 1 : 0;          // the window starts an episode
    }
}

hipError_t rck_sample_windows(const RcSampleWindows &a, hipStream_t s) {
    hipLaunchKernelGGL(rc_sample_windows_kernel, dim3((unsigned)((a.n_windows + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- flags of the peer-copy all-gather (rc_gather_trajectory_p2p): sequence numbers in uncached device memory that a
// PEER's kernel writes (over xGMI) and the owner's kernel polls.  Both kernels are one wave; the poll is bounded (wall
// clock) and reports a time-out instead of hanging the queue.
__global__ __launch_bounds__(64) void rc_p2p_post_kernel(RcP2pPost post) {
    // lane p stores `value` into flag p (a pointer into peer p's flag block, or null)
    const unsigned l = threadIdx.x;
    if (l < (unsigned)post.n && post.flag[l] != nullptr)
        __hip_atomic_store(post.flag[l], post.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(64) void rc_p2p_wait_kernel(const uint32_t *flags, int n, int skip, uint32_t value, uint32_t *timeouts,
                                                         unsigned long long limit_ticks) {
    // lane p waits until flags[p] >= value (sequence numbers only grow); every lane leaves the loop at the deadline
    const unsigned l = threadIdx.x;
    const unsigned long long t0 = wall_clock64();
    bool late = false;
    if (l < (unsigned)n && (int)l != skip) {
        while (__hip_atomic_load(flags + l, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < value) {
            if (wall_clock64() - t0 > limit_ticks) { late = true; break; }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (late) atomicAdd(timeouts, 1u);
}

hipError_t rck_p2p_post(const RcP2pPost &post, hipStream_t s) {
    hipLaunchKernelGGL(rc_p2p_post_kernel, dim3(1), dim3(64), 0, s, post);
    return hipGetLastError();
}

hipError_t rck_p2p_wait(const uint32_t *flags, int n, int skip, uint32_t value, uint32_t *timeouts, double limit_s, hipStream_t s) {
    hipLaunchKernelGGL(rc_p2p_wait_kernel, dim3(1), dim3(64), 0, s, flags, n, skip, value, timeouts,
                       (unsigned long long)(limit_s * 1.0e8));        // wall_clock64 counts at 100 MHz
    return hipGetLastError();
}

struct RcUid { char internal[128]; };      // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value

// ---- RCCL, bound at run time (rc_comm_init): the library has no link-time dependency on it, so single-GPU clients
// need no RCCL installed, and a process that already holds a copy (PyTorch bundles one) keeps using that copy.
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value */ struct RcUid, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};

// ---- peer-copy all-gather (on the xGMI full mesh every shard crosses exactly one link once if each rank
// copies its record straight into every peer's buffer - N - 1 concurrent copies - where a ring passes it N - 1 times).
// Every rank owns: the destination, two slots of world x bytes (hipMalloc, exported over hipIpc), and a block of
// sequence flags in uncached device memory that its PEERS write: arrived[p] = k + 1 when peer p's shard of gather k has
// landed, released[p] = k + 1 when peer p allows gather k to be written into ITS slot k & 1.
struct P2pExport {                 // what a rank hands to its peers (RC_P2P_EXPORT_BYTES)
    hipIpcMemHandle_t dst, flags;
    uint64_t bytes;                // per rank and slot
    int32_t rank, world, mode, pid;
    char pci[32];
    char pad[RC_P2P_EXPORT_BYTES - 2 * sizeof(hipIpcMemHandle_t) - 8 - 16 - 32];
};
static_assert(sizeof(P2pExport) == RC_P2P_EXPORT_BYTES, "export blob size");

struct P2p {
    int rank = 0, world = 0, mode = 0;
    size_t bytes = 0;              // one rank's record in the current mode
    size_t cap = 0;                // ... and in the largest one (RC_GATHER_FULL): what the slots are sized for
    P2pExport blob{};              // what rc_p2p_setup handed out
    char *dst = nullptr;           // [2][world][cap], mine
    uint32_t *flags = nullptr;     // arrived[64] | released[64] | timeouts, mine (uncached)
    std::vector<char *> peer_dst;          // peers' destinations, opened (null for me)
    std::vector<uint32_t *> peer_flags;    // peers' flag blocks, opened (null for me)
    std::vector<hipStream_t> push;         // one stream per peer (the local copy runs on push[rank])
    hipStream_t ctrl = nullptr;            // release + wait-for-release kernels; arrival waits
    hipEvent_t ev_ready = nullptr, ev_go = nullptr, ev_arrived = nullptr, ev_local = nullptr;
    std::vector<hipEvent_t> ev_sent;       // per peer: my copy into its slot and the arrival flag behind it have been executed
    uint32_t issued = 0;           // gathers issued so far
    bool connected = false;
    uint32_t *arrived() const { return flags; }
    uint32_t *released() const { return flags + RC_P2P_MAX_RANKS; }
    uint32_t *timeouts() const { return flags + 2 * RC_P2P_MAX_RANKS; }
};

namespace {

Rccl g_rccl;
std::string g_rccl_path;
std::mutex g_rccl_mutex;

int load_rccl() {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);       // handles may be set up from different threads
    if (g_rccl.handle) return RC_OK;
    void *h = nullptr;
    if (!g_rccl_path.empty()) {
        h = dlopen(g_rccl_path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(RC_ERR_COMM, "dlopen(%s) failed: %s", g_rccl_path.c_str(), dlerror());
    } else {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char *n : names)                       // a copy the process already holds wins
            if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) break;
        if (!h)
            for (const char *n : names)
                if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return fail(RC_ERR_COMM, "RCCL not found (tried librccl.so.1, librccl.so, /opt/rocm/lib): %s", dlerror());
    }
    Rccl r;
    r.handle = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.CommCount = (decltype(r.CommCount))dlsym(h, "ncclCommCount");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString)
        return fail(RC_ERR_COMM, "the RCCL library lacks an expected symbol");
    g_rccl = r;
    return RC_OK;
}

#define NCCL_TRY(expr)                                                                                     \
    do {                                                                                                   \
        int _r = (expr);                                                                                   \
        if (_r != 0) return fail(RC_ERR_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(_r));          \
    } while (0)

// source pointer and size of what one gather mode sends
int gather_source(rc_env *env, int mode, const void **src, size_t *bytes) {
    switch (mode) {
    case RC_GATHER_FULL:
        if (env->shared_arena) return fail(RC_ERR_INVALID, "this handle fills a slice of a shared arena: gather the arena itself");
        *src = env->out_arena;
        *bytes = env->layout.slab_bytes;
        return RC_OK;
    case RC_GATHER_SUMMARY:
        if (env->shared_arena) return fail(RC_ERR_INVALID, "this handle fills a slice of a shared arena: gather the arena itself");
        *src = (const char *)env->out_arena + env->compact.summary_src_off;
        *bytes = env->compact.summary_bytes;
        return RC_OK;
    case RC_GATHER_FULL_U16:
        if (!env->compact_slab) return fail(RC_ERR_INVALID, "RC_GATHER_FULL_U16 needs rc_set_compact_slab first");
        *src = env->compact_slab;
        *bytes = env->compact.total;
        return RC_OK;
    }
    return fail(RC_ERR_INVALID, "unknown gather mode %d", mode);
}

}  // namespace

// ---- peer-copy all-gather ------------------------------------------------------------------------------------------
static void p2p_disconnect(rc_env *env) {          // my copies done, the peers' buffers unmapped; mine stay
    P2p *x = env->p2p;
    if (!x) return;
    (void)hipSetDevice(env->cfg.device);
    for (hipStream_t st : x->push) if (st) { (void)hipStreamSynchronize(st); }
    if (x->ctrl) (void)hipStreamSynchronize(x->ctrl);
    for (char *&d : x->peer_dst) if (d) { (void)hipIpcCloseMemHandle(d); d = nullptr; }
    for (uint32_t *&f : x->peer_flags) if (f) { (void)hipIpcCloseMemHandle(f); f = nullptr; }
    x->connected = false;
}

static void p2p_free(rc_env *env) {
    P2p *x = env->p2p;
    if (!x) return;
    p2p_disconnect(env);
    for (hipStream_t st : x->push) if (st) (void)hipStreamDestroy(st);
    if (x->ctrl) (void)hipStreamDestroy(x->ctrl);
    for (hipEvent_t e : {x->ev_ready, x->ev_go, x->ev_arrived, x->ev_local}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : x->ev_sent) if (e) (void)hipEventDestroy(e);
    if (x->dst) (void)hipFree(x->dst);
    if (x->flags) (void)hipFree(x->flags);
    delete x;
    env->p2p = nullptr;
}

void gather_release(rc_env *env) {
    p2p_free(env);
    if (env->comm_stream) (void)hipStreamSynchronize(env->comm_stream);
    if (env->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(env->comm);
    if (env->ev_ready) (void)hipEventDestroy(env->ev_ready);
    if (env->ev_gathered) (void)hipEventDestroy(env->ev_gathered);
    if (env->comm_stream) (void)hipStreamDestroy(env->comm_stream);
}

extern "C" {

namespace {
// The field table of a row gather: for every field of the mask, in field order, where its section starts in an arena, where its
// rows go in the output (sections of `n_rows` rows, 64-byte aligned) and its bytes per car; `total` is the output's size.
// `bad` is the first field of the mask that a recorded arena of this configuration does not hold (the action input buffer, a
// section that is off), or -1: such a mask is refused by every caller but rc_gather_rows_bytes, which has no error to return.
struct GatherFields {
    size_t src[RC_GATHER_MAX_FIELDS], dst[RC_GATHER_MAX_FIELDS], total;
    uint32_t bpc[RC_GATHER_MAX_FIELDS];
    int field[RC_GATHER_MAX_FIELDS], n, bad;
};
GatherFields gather_fields(const rc_env *env, uint32_t field_mask, size_t n_rows) {
    GatherFields g{};
    g.bad = -1;
    for (int f = 0; f < RC_F_COUNT; ++f) {
        if (!((field_mask >> f) & 1u)) continue;
        if ((f == RC_F_ACTION_IN || !env->layout.bytes[f]) && g.bad < 0) g.bad = f;
        if (!env->layout.bytes[f]) continue;
        g.field[g.n] = f; g.src[g.n] = env->layout.offset[f]; g.dst[g.n] = g.total; g.bpc[g.n] = (uint32_t)kFieldBytes[f];
        g.total = align_up(g.total + kFieldBytes[f] * n_rows, 64);
        ++g.n;
    }
    return g;
}

// what rc_gather_rows and rc_sample_windows ask of a ring of recorded arenas
int check_ring(const rc_env *env, const void *ring_base, size_t slot_bytes, const char *who) {
    if (slot_bytes < env->layout.total) return fail(RC_ERR_INVALID, "slot_bytes %zu is smaller than an arena (%zu)", slot_bytes, env->layout.total);
    // (the row gather moves 16 bytes per lane: every slot must start as rc_set_arena demands of an arena)
    if (((uintptr_t)ring_base & 63u) != 0 || (slot_bytes & 63u) != 0)
        return fail(RC_ERR_INVALID, "ring_base (%p) and slot_bytes (%zu) must be multiples of 64", ring_base, slot_bytes);
    if (env->shared_arena) return fail(RC_ERR_INVALID, "%s works on whole arenas, not on a slice handle", who);
    return RC_OK;
}
}  // namespace

size_t rc_gather_rows_bytes(rc_env *env, uint32_t field_mask, int32_t n_rows) {
    if (!env || n_rows < 1) return 0;
    return gather_fields(env, field_mask, (size_t)n_rows).total;
}

int rc_gather_rows(rc_env *env, const void *ring_base, size_t slot_bytes, const int32_t *slot_idx_dev, const int32_t *car_idx_dev,
                   int32_t n_rows, uint32_t field_mask, void *out_dev, size_t out_bytes) {
    if (!env || !ring_base || !slot_idx_dev || !car_idx_dev || !out_dev) return fail(RC_ERR_INVALID, "NULL argument");
    if (n_rows < 1) return fail(RC_ERR_INVALID, "n_rows must be >= 1");
    int rc = check_ring(env, ring_base, slot_bytes, "rc_gather_rows");
    if (rc) return rc;
    const GatherFields g = gather_fields(env, field_mask, (size_t)n_rows);
    if (g.bad >= 0) return fail(RC_ERR_INVALID, "field %d is not part of a recorded arena in this configuration", g.bad);
    if (g.n == 0) return fail(RC_ERR_INVALID, "empty field mask");
    if (out_bytes < g.total) return fail(RC_ERR_INVALID, "output too small: %zu < %zu", out_bytes, g.total);
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(rck_gather_rows(ring_base, slot_bytes, slot_idx_dev, car_idx_dev, n_rows, g.src, g.dst, g.bpc, g.n, out_dev, env->stream));
    return RC_OK;
}

int rc_sample_windows(rc_env *env, const void *ring_base, size_t slot_bytes, int32_t capacity, int32_t oldest, int32_t count,
                      int32_t length, int32_t n_windows, uint64_t seed, uint32_t draw, int32_t max_tries, int32_t *slot_idx_dev,
                      int32_t *slot_obs_idx_dev, int32_t *car_idx_dev, int32_t *meta_dev, uint32_t *failed_dev) {
    if (!env || !ring_base || !slot_idx_dev || !slot_obs_idx_dev || !car_idx_dev || !meta_dev || !failed_dev) return fail(RC_ERR_INVALID, "NULL argument");
    int rc = check_ring(env, ring_base, slot_bytes, "rc_sample_windows");
    if (rc) return rc;
    if (capacity < 1 || oldest < 0 || oldest >= capacity || count < 1 || count > capacity) return fail(RC_ERR_INVALID, "ring of %d slots, oldest %d, %d filled", capacity, oldest, count);
    if (length < 1 || length > count) return fail(RC_ERR_INVALID, "a window of %d records does not fit the %d records of the ring", length, count);
    if (n_windows < 1 || max_tries < 1) return fail(RC_ERR_INVALID, "n_windows and max_tries must be >= 1");
    RcSampleWindows a{};
    a.ring = (const unsigned char *)ring_base; a.slot_bytes = slot_bytes;
    a.fresh_off = env->layout.offset[RC_F_FRESH]; a.done_off = env->layout.offset[RC_F_DONE];
    a.capacity = capacity; a.oldest = oldest; a.n_start = count - length + 1; a.length = length; a.n_windows = n_windows;
    a.n_cars = env->n_cars; a.max_tries = max_tries;
    a.seed_lo = seed_lo(seed); a.seed_hi = seed_hi(seed); a.draw = draw;
    a.slot_idx = slot_idx_dev; a.slot_obs_idx = slot_obs_idx_dev; a.car_idx = car_idx_dev; a.meta = meta_dev; a.failed = failed_dev;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(rck_sample_windows(a, env->stream));
    return RC_OK;
}

// One training batch as ONE packed buffer: field sections (64-byte aligned, field order), meta, the failure counter - the
// payload a sharded replay store exchanges - then the sampler's row indices (scratch).
namespace {
struct BatchLayout { GatherFields fields; size_t meta, failed, payload, slot, slot_obs, car, total; };
bool batch_layout(const rc_env *env, uint32_t field_mask, int32_t n_windows, int32_t length, BatchLayout *bl) {
    const size_t rows = (size_t)n_windows * (size_t)length;
    bl->fields = gather_fields(env, field_mask, rows);
    if (bl->fields.bad >= 0) return false;
    size_t off = bl->fields.total;
    bl->meta = off;     off = align_up(off + 16u * (size_t)n_windows, 64);
    bl->failed = off;   off += 64;
    bl->payload = off;
    bl->slot = off;     off = align_up(off + 4u * rows, 64);
    bl->slot_obs = off; off = align_up(off + 4u * rows, 64);
    bl->car = off;      off = align_up(off + 4u * rows, 64);
    bl->total = off;
    return true;
}
}  // namespace

size_t rc_sample_batch_bytes(rc_env *env, uint32_t field_mask, int32_t n_windows, int32_t length, size_t *payload_bytes, size_t *meta_offset) {
    if (!env || n_windows < 1 || length < 1 || field_mask == 0u) return 0;
    BatchLayout bl;
    if (!batch_layout(env, field_mask, n_windows, length, &bl)) return 0;
    if (payload_bytes) *payload_bytes = bl.payload;
    if (meta_offset) *meta_offset = bl.meta;
    return bl.total;
}

int rc_sample_batch(rc_env *env, const void *ring_base, size_t slot_bytes, int32_t capacity, int32_t oldest, int32_t count, int32_t length,
                    int32_t n_windows, uint64_t seed, uint32_t draw, int32_t max_tries, uint32_t field_mask, int32_t reset_rows,
                    void *out_dev, size_t out_bytes) {
    if (!env || !ring_base || !out_dev) return fail(RC_ERR_INVALID, "NULL argument");
    if (n_windows < 1 || length < 1) return fail(RC_ERR_INVALID, "n_windows and length must be >= 1");
    BatchLayout bl;
    if (field_mask == 0u || !batch_layout(env, field_mask, n_windows, length, &bl))
        return fail(RC_ERR_INVALID, "field mask 0x%x names no field, or one that is not part of a recorded arena in this configuration", field_mask);
    if (out_bytes < bl.total) return fail(RC_ERR_INVALID, "output too small: %zu < %zu (rc_sample_batch_bytes)", out_bytes, bl.total);
    if (((uintptr_t)out_dev & 63u) != 0) return fail(RC_ERR_INVALID, "out_dev must be 64-byte aligned");
    char *out = (char *)out_dev;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipMemsetAsync(out + bl.failed, 0, 64, env->stream));
    int rc = rc_sample_windows(env, ring_base, slot_bytes, capacity, oldest, count, length, n_windows, seed, draw, max_tries,
                               (int32_t *)(out + bl.slot), (int32_t *)(out + bl.slot_obs), (int32_t *)(out + bl.car),
                               (int32_t *)(out + bl.meta), (uint32_t *)(out + bl.failed));
    if (rc) return rc;
    // the observation part of a record: what a terminal row borrows from the row before it
    const uint32_t obs_fields = (1u << RC_F_LIDAR) | (1u << RC_F_OCCUPANCY) | (1u << RC_F_POSE) | (1u << RC_F_VELOCITY) | (1u << RC_F_SPEED) |
                                (1u << RC_F_ACCELERATION) | (1u << RC_F_STEERING_ANGLE);
    const GatherFields &g = bl.fields;
    RcBatchRows br{};
    br.slot_obs_idx = (const int32_t *)(out + bl.slot_obs); br.meta = (const int32_t *)(out + bl.meta); br.length = length;
    for (int i = 0; i < g.n; ++i) {
        const int f = g.field[i];
        if ((obs_fields >> f) & 1u) br.obs_mask |= 1u << i;
        if (reset_rows && (f == RC_F_ACTION || f == RC_F_REWARD || f == RC_F_DISCOUNT || f == RC_F_TIME || f == RC_F_PROGRESS_TOTAL)) {
            const float v = f == RC_F_DISCOUNT ? 1.0f : (f == RC_F_PROGRESS_TOTAL ? -1.0f : 0.0f);
            br.reset_mask |= 1u << i;
            std::memcpy(&br.reset_word[i], &v, 4);
        }
    }
    HIP_TRY(rck_gather_rows(ring_base, slot_bytes, (const int32_t *)(out + bl.slot), (const int32_t *)(out + bl.car), n_windows * length,
                            g.src, g.dst, g.bpc, g.n, out, env->stream, &br));
    return RC_OK;
}

int rc_comm_library(const char *path) {
    if (g_rccl.handle) return fail(RC_ERR_INVALID, "RCCL is already loaded");
    g_rccl_path = path ? path : "";
    return RC_OK;
}

int rc_comm_unique_id(void *out, size_t bytes) {
    if (!out || bytes < sizeof(RcUid)) return fail(RC_ERR_INVALID, "unique id buffer must hold %zu bytes", sizeof(RcUid));
    int rc = load_rccl();
    if (rc) return rc;
    NCCL_TRY(g_rccl.GetUniqueId(out));
    return RC_OK;
}

int rc_comm_init(rc_env *env, const void *unique_id, size_t bytes, int32_t rank, int32_t world) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!unique_id || bytes < sizeof(RcUid)) return fail(RC_ERR_INVALID, "unique id must hold %zu bytes", sizeof(RcUid));
    if (world < 1 || rank < 0 || rank >= world) return fail(RC_ERR_INVALID, "rank %d outside world of %d", rank, world);
    if (env->comm) return fail(RC_ERR_INVALID, "the handle already has a communicator");
    int rc = load_rccl();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcUid id;
    std::memcpy(&id, unique_id, sizeof(id));
    NCCL_TRY(g_rccl.CommInitRank(&env->comm, world, id, rank));
    env->comm_rank = rank;
    env->comm_world = world;
    HIP_TRY(hipStreamCreateWithFlags(&env->comm_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&env->ev_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&env->ev_gathered, hipEventDisableTiming));
    return RC_OK;
}

int rc_comm_count(rc_env *env, int32_t *ranks) {
    if (!env || !ranks) return fail(RC_ERR_INVALID, "NULL argument");
    if (!env->comm) return fail(RC_ERR_INVALID, "rc_comm_init has not been called on this handle");
    if (!g_rccl.CommCount) return fail(RC_ERR_COMM, "the RCCL library lacks ncclCommCount");
    int n = 0;
    NCCL_TRY(g_rccl.CommCount(env->comm, &n));
    *ranks = n;
    return RC_OK;
}

size_t rc_gather_bytes(rc_env *env, int32_t mode) {
    if (!env) return 0;
    switch (mode) {
    case RC_GATHER_FULL: return env->layout.slab_bytes;
    case RC_GATHER_FULL_U16: return env->compact.total;
    case RC_GATHER_SUMMARY: return env->compact.summary_bytes;
    }
    return 0;
}

int rc_gather_trajectory(rc_env *env, int32_t mode, void *dev_dst, size_t dst_bytes) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->comm) return fail(RC_ERR_INVALID, "rc_comm_init has not been called on this handle");
    if (!dev_dst) return fail(RC_ERR_INVALID, "dev_dst is NULL");
    const void *src;
    size_t n;
    int rc = gather_source(env, mode, &src, &n);
    if (rc) return rc;
    if (dst_bytes < n * (size_t)env->comm_world)
        return fail(RC_ERR_INVALID, "gather destination too small: %zu < %d x %zu", dst_bytes, env->comm_world, n);
    HIP_TRY(hipSetDevice(env->cfg.device));
    // ordered after everything queued on the env's stream (the step that produced the record), but on a stream of
    // its own: the following steps' kernels overlap the collective
    HIP_TRY(hipEventRecord(env->ev_ready, env->stream));
    HIP_TRY(hipStreamWaitEvent(env->comm_stream, env->ev_ready, 0));
    NCCL_TRY(g_rccl.AllGather(src, dev_dst, n, /* ncclUint8 */ 1, env->comm, env->comm_stream));
    HIP_TRY(hipEventRecord(env->ev_gathered, env->comm_stream));
    env->gather_pending = true;
    return RC_OK;
}

int rc_gather_wait(rc_env *env, int32_t host_sync) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->gather_pending) return RC_OK;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamWaitEvent(env->stream, env->ev_gathered, 0));     // later work on the env's stream sees the result
    if (host_sync) {
        HIP_TRY(hipEventSynchronize(env->ev_gathered));
        env->gather_pending = false;
    }
    return RC_OK;
}

int rc_p2p_setup(rc_env *env, int32_t mode, int32_t rank, int32_t world, void *export_out, size_t bytes) {
    if (!env || !export_out) return fail(RC_ERR_INVALID, "NULL argument");
    if (bytes < RC_P2P_EXPORT_BYTES) return fail(RC_ERR_INVALID, "export buffer must hold %d bytes", RC_P2P_EXPORT_BYTES);
    if (world < 1 || world > RC_P2P_MAX_RANKS || rank < 0 || rank >= world)
        return fail(RC_ERR_INVALID, "rank %d outside world of %d (at most %d ranks)", rank, world, RC_P2P_MAX_RANKS);
    const size_t n = rc_gather_bytes(env, mode);
    if (n == 0) return fail(RC_ERR_INVALID, "unknown gather mode %d", mode);
    HIP_TRY(hipSetDevice(env->cfg.device));
    if (P2p *x = env->p2p) {
        // Already set up: only the payload changes.  The buffers, their exports and the peers' mappings stay - they are
        // sized for the largest payload, and exporting fresh allocations again and again is what the runtime likes least
        // (a re-export at a recycled address failed with "invalid argument" now and then).  Sequence numbers run on.
        if (x->rank != rank || x->world != world) return fail(RC_ERR_INVALID, "set up as rank %d of %d: rc_p2p_teardown first", x->rank, x->world);
        for (hipStream_t st : x->push) HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipStreamSynchronize(x->ctrl));
        x->mode = mode; x->bytes = n;
        std::memcpy(export_out, &x->blob, sizeof(x->blob));
        return RC_OK;
    }
    P2p *x = new (std::nothrow) P2p();
    if (!x) return fail(RC_ERR_NOMEM, "out of host memory");
    env->p2p = x;
    x->rank = rank; x->world = world; x->mode = mode; x->bytes = n;
    x->cap = align_up(std::max(n, env->layout.slab_bytes), 256);
    x->peer_dst.assign(world, nullptr);
    x->peer_flags.assign(world, nullptr);
    x->push.assign(world, nullptr);
    x->ev_sent.assign(world, nullptr);
#define P2P_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { p2p_free(env); return fail(RC_ERR_HIP, "%s failed: %s (payload %zu B x %d ranks)", #expr, hipGetErrorString(_e), n, world); } } while (0)
    P2P_TRY(hipMalloc((void **)&x->dst, 2 * (size_t)world * x->cap));
    // the flags are written by other GPUs' kernels and polled by this one's: uncached memory, so that a poll sees them
    P2P_TRY(hipExtMallocWithFlags((void **)&x->flags, 4096, hipDeviceMallocUncached));
    P2P_TRY(hipMemset(x->flags, 0, 4096));
    for (int p = 0; p < world; ++p) P2P_TRY(hipStreamCreateWithFlags(&x->push[p], hipStreamNonBlocking));
    P2P_TRY(hipStreamCreateWithFlags(&x->ctrl, hipStreamNonBlocking));
    for (hipEvent_t *e : {&x->ev_ready, &x->ev_go, &x->ev_arrived, &x->ev_local}) P2P_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (int p = 0; p < world; ++p) if (p != rank) P2P_TRY(hipEventCreateWithFlags(&x->ev_sent[p], hipEventDisableTiming));
    P2pExport &ex = x->blob;
    std::memset(&ex, 0, sizeof(ex));
    P2P_TRY(hipIpcGetMemHandle(&ex.dst, x->dst));
    P2P_TRY(hipIpcGetMemHandle(&ex.flags, x->flags));
    ex.bytes = x->cap; ex.rank = rank; ex.world = world; ex.mode = 0; ex.pid = (int32_t)getpid();
    P2P_TRY(hipDeviceGetPCIBusId(ex.pci, sizeof(ex.pci), env->cfg.device));
    std::memcpy(export_out, &ex, sizeof(ex));
    return RC_OK;
}

int rc_p2p_connect(rc_env *env, const void *exports, size_t bytes) {
    if (!env || !exports) return fail(RC_ERR_INVALID, "NULL argument");
    P2p *x = env->p2p;
    if (!x) return fail(RC_ERR_INVALID, "rc_p2p_setup has not been called on this handle");
    if (x->connected) return RC_OK;                      // (a mode switch: the peers' buffers are mapped already)
    if (bytes < (size_t)x->world * RC_P2P_EXPORT_BYTES) return fail(RC_ERR_INVALID, "need %d export blobs of %d bytes", x->world, RC_P2P_EXPORT_BYTES);
    HIP_TRY(hipSetDevice(env->cfg.device));
    for (int p = 0; p < x->world; ++p) {
        P2pExport ex;
        std::memcpy(&ex, (const char *)exports + (size_t)p * RC_P2P_EXPORT_BYTES, sizeof(ex));
        if (ex.rank != p || ex.world != x->world || ex.bytes != x->cap) {
            p2p_disconnect(env);
            return fail(RC_ERR_INVALID, "export blob %d does not match (rank %d, world %d, %llu bytes per slot entry; mine %zu)", p, ex.rank, ex.world,
                        (unsigned long long)ex.bytes, x->cap);
        }
        if (p == x->rank) continue;
        // a peer on another GPU: let this device's copy engines and kernels reach its memory
        int pdev = -1;
        if (hipDeviceGetByPCIBusId(&pdev, ex.pci) == hipSuccess && pdev >= 0 && pdev != env->cfg.device) {
            hipError_t pe = hipDeviceEnablePeerAccess(pdev, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
                p2p_disconnect(env);
                return fail(RC_ERR_HIP, "hipDeviceEnablePeerAccess(%d) failed: %s", pdev, hipGetErrorString(pe));
            }
            (void)hipGetLastError();
        }
        // (a failure half way leaves nothing mapped: the call can be repeated)
        hipError_t oe = hipIpcOpenMemHandle((void **)&x->peer_dst[p], ex.dst, hipIpcMemLazyEnablePeerAccess);
        if (oe == hipSuccess) oe = hipIpcOpenMemHandle((void **)&x->peer_flags[p], ex.flags, hipIpcMemLazyEnablePeerAccess);
        if (oe != hipSuccess) {
            p2p_disconnect(env);
            return fail(RC_ERR_HIP, "hipIpcOpenMemHandle of rank %d's buffers failed: %s", p, hipGetErrorString(oe));
        }
    }
    x->connected = true;
    return RC_OK;
}

int rc_gather_trajectory_p2p(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    P2p *x = env->p2p;
    if (!x || !x->connected) return fail(RC_ERR_INVALID, "rc_p2p_setup / rc_p2p_connect have not been called on this handle");
    const void *src;
    size_t n;
    int rc = gather_source(env, x->mode, &src, &n);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(env->cfg.device));
    const uint32_t k = x->issued, seq = k + 1u;
    // slot k & 1 of every rank: world entries of `cap` bytes, of which the current payload fills the first n
    const size_t slot_off = (size_t)(k & 1u) * x->world * x->cap, mine = slot_off + (size_t)x->rank * x->cap;
    // everything below is ordered behind what the env's stream holds now: the step that produced the record, and the
    // caller's use of the slot that gather k overwrites (the buffer of gather k - 2)
    HIP_TRY(hipEventRecord(x->ev_ready, env->stream));
    HIP_TRY(hipStreamWaitEvent(x->ctrl, x->ev_ready, 0));
    // 1. tell every peer that its gather k may be written into my slot k & 1 ...
    RcP2pPost post;
    std::memset(&post, 0, sizeof(post));
    post.n = x->world; post.value = seq;
    for (int p = 0; p < x->world; ++p) post.flag[p] = p == x->rank ? nullptr : x->peer_flags[p] + RC_P2P_MAX_RANKS + x->rank;
    HIP_TRY(rck_p2p_post(post, x->ctrl));
    // 2. ... and wait until every peer has said the same to me (posting comes first on every rank: no cycle)
    HIP_TRY(rck_p2p_wait(x->released(), x->world, x->rank, seq, x->timeouts(), RC_P2P_TIMEOUT_S, x->ctrl));
    HIP_TRY(hipEventRecord(x->ev_go, x->ctrl));
    // 3. my record into every peer's slot, one stream (one link) per peer, each followed by its arrival flag
    for (int p = 0; p < x->world; ++p) {
        hipStream_t st = x->push[p];
        if (p == x->rank) {
            HIP_TRY(hipStreamWaitEvent(st, x->ev_ready, 0));
            HIP_TRY(hipMemcpyAsync(x->dst + mine, src, n, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipEventRecord(x->ev_local, st));
            continue;
        }
        HIP_TRY(hipStreamWaitEvent(st, x->ev_go, 0));
        HIP_TRY(hipMemcpyAsync(x->peer_dst[p] + mine, src, n, hipMemcpyDefault, st));
        RcP2pPost arrived;
        std::memset(&arrived, 0, sizeof(arrived));
        arrived.n = 1; arrived.value = seq;
        arrived.flag[0] = x->peer_flags[p] + x->rank;
        HIP_TRY(rck_p2p_post(arrived, st));
        HIP_TRY(hipEventRecord(x->ev_sent[p], st));
    }
    // 4. arrival of every peer's shard in my slot: polled on the control stream, behind the release handshake
    HIP_TRY(rck_p2p_wait(x->arrived(), x->world, x->rank, seq, x->timeouts(), RC_P2P_TIMEOUT_S, x->ctrl));
    HIP_TRY(hipStreamWaitEvent(x->ctrl, x->ev_local, 0));
    // 5. ... and the DEPARTURE of mine: `ev_arrived` stands for "gather k is complete as far as this rank can tell" - the peers'
    // shards are here AND my outbound copies have read the source to the end - so that a caller who puts its stream behind it
    // (rc_gather_p2p_wait, host_sync 0) may let the next step but one rewrite the source, as with rc_gather_trajectory
    for (int p = 0; p < x->world; ++p) if (p != x->rank) HIP_TRY(hipStreamWaitEvent(x->ctrl, x->ev_sent[p], 0));
    HIP_TRY(hipEventRecord(x->ev_arrived, x->ctrl));
    x->issued = seq;
    return RC_OK;
}

int rc_gather_p2p_wait(rc_env *env, int32_t host_sync, void **gathered_dev, size_t *gathered_bytes) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    P2p *x = env->p2p;
    if (!x || !x->connected) return fail(RC_ERR_INVALID, "rc_p2p_setup / rc_p2p_connect have not been called on this handle");
    if (x->issued == 0) return fail(RC_ERR_INVALID, "no gather has been issued");
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamWaitEvent(env->stream, x->ev_arrived, 0));       // later work on the env's stream sees the gathered bytes
    if (host_sync) {
        HIP_TRY(hipEventSynchronize(x->ev_arrived));
        // my record has left when my copies are done (the peers' arrival flags follow them on the same streams)
        for (int p = 0; p < x->world; ++p) HIP_TRY(hipStreamSynchronize(x->push[p]));
        uint32_t late = 0;
        HIP_TRY(hipMemcpy(&late, x->timeouts(), sizeof(late), hipMemcpyDeviceToHost));
        if (late != 0) {
            // reported once: the counter starts again (everything queued has run: the streams were synchronised above).  A
            // release wait that timed out has let its copies go into slots that were never released: the records of this
            // and of the previous gather are not to be trusted, on any rank - tear the transport down and set it up again
            HIP_TRY(hipMemset(x->timeouts(), 0, sizeof(uint32_t)));
            return fail(RC_ERR_COMM, "peer-copy gather: %u flag wait(s) timed out after %.0f s (a peer did not post); the gathered "
                        "slots are not valid - rc_p2p_teardown and set up again", late, (double)RC_P2P_TIMEOUT_S);
        }
    }
    if (gathered_dev) *gathered_dev = x->dst + (size_t)((x->issued - 1u) & 1u) * x->world * x->cap;
    if (gathered_bytes) *gathered_bytes = (size_t)x->world * x->cap;
    return RC_OK;
}

int rc_p2p_slot(rc_env *env, int32_t back, void **gathered_dev, size_t *gathered_bytes) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    P2p *x = env->p2p;
    if (!x) return fail(RC_ERR_INVALID, "rc_p2p_setup has not been called on this handle");
    if (back < 0 || back > 1 || x->issued < (uint32_t)back + 1u) return fail(RC_ERR_INVALID, "no gather %d before the last one (issued: %u)", back, x->issued);
    if (gathered_dev) *gathered_dev = x->dst + (size_t)((x->issued - 1u - (uint32_t)back) & 1u) * x->world * x->cap;
    if (gathered_bytes) *gathered_bytes = (size_t)x->world * x->cap;
    return RC_OK;
}

int rc_p2p_disconnect(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    p2p_disconnect(env);
    return RC_OK;
}

int rc_p2p_teardown(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    p2p_free(env);
    return RC_OK;
}

}  // extern "C"
