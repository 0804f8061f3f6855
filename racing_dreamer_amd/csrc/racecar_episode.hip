// The episode log (include/racecar_hip.h, rc_episode_log_*): per-car running sums of the episode on the device and, in the
// call in which an env's episode ends, one row per car appended to a fixed-size buffer in (call, env, slot) order - what
// the reference's summarize_episode / summarize_eval_episode compute on the host from the recorded episode
// (dreamer/callbacks.py:56-100: return = reward.sum(), length = len(reward) - 1, progress = max(progress), time = max(time)).
//
// The kernels only READ what the dynamics left in the output arena (store_step_results: the terminal values in the call
// that ends an episode, also under auto-reset; store_state_and_obs: fresh = 1 when the env was respawned in that call) and
// the env's current track; everything they write is the handle's own log memory.  No kernel of the step is touched.
//
// Order.  The rows of one call must come out by env, then slot - not in the order in which waves happen to arrive, which
// differs from run to run.  So the positions are an exclusive prefix sum over the envs of "this env logs in this call":
//   rc_episode_count_kernel   one env per lane: ballot + popcount per wave, the workgroup's count to block_counts[b]
//   rc_episode_update_kernel  every workgroup sums the counts of the workgroups before it (256 words at 65 536 envs: one load
//                             per lane) and the total, ranks its own envs with ballot + mbcnt, then accumulates, writes the
//                             rows of its ending envs at cursor + rank * cars_per_env + slot, and re-arms or freezes them
// Two launches and no wait of one workgroup for another: a single-launch look-back would save a launch gap at the price of
// workgroups spinning on each other's flags (EXPERIMENTS.md).  Both kernels evaluate the same predicate (ep_logs) on state
// that only the second one changes.  The running row cursor is kept twice, by call parity: every workgroup reads
// cursor[call & 1], workgroup 0 writes cursor[(call + 1) & 1] - no workgroup can see the value of the next call.
// Sums that do not depend on order (skipped, abandoned, envs_at_quota) are 64-bit atomicAdd, one per wave.
#include "racecar_env.h"

namespace {

__device__ __forceinline__ bool ep_any_done(const RcEpisodeDev &d, int e) {
    bool any = false;
    for (int a = 0; a < d.cars_per_env; ++a) any |= d.done[e * d.cars_per_env + a] != 0;
    return any;
}

// the env's episode ends in this call, it was followed from its start, and it is within the per-env quota: its cars get rows
// (or are counted as dropped if the buffer is full)
__device__ __forceinline__ bool ep_logs(const RcEpisodeDev &d, int e) {
    if (!d.active[e] || !ep_any_done(d, e)) return false;
    return d.max_episodes == 0u || d.ordinal[e] < d.max_episodes;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

__device__ __forceinline__ void ep_start(const RcEpisodeDev &d, int e) {
    const int A = d.cars_per_env;
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        d.ret[i] = 0.0f;            // the reset row: reward 0, progress -1, time 0 (dreamer/wrappers.py:232-236)
        d.prog_max[i] = -1.0f;
        d.time_max[i] = 0.0f;
        d.wrong_seen[i] = 0;
    }
    int k = 0;
    if (d.ts_track != nullptr) {
        k = d.ts_track[e];
        k = (unsigned)k < (unsigned)d.ts_n ? k : 0;      // as ts_track_of (racecar_kernels.hip)
    }
    d.track[e] = k;
    d.length[e] = 0;
    d.active[e] = 1;
}

__global__ __launch_bounds__(RC_EP_BLOCK) void rc_episode_count_kernel(RcEpisodeDev d) {
    __shared__ uint32_t s_wave[RC_EP_BLOCK / 64];
    const int e = blockIdx.x * RC_EP_BLOCK + threadIdx.x;
    const bool logs = e < d.num_envs && ep_logs(d, e);
    const unsigned long long b = __ballot(logs);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < RC_EP_BLOCK / 64; ++w) n += s_wave[w];
        d.block_counts[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(RC_EP_BLOCK) void rc_episode_update_kernel(RcEpisodeDev d) {
    __shared__ uint32_t s_pre[RC_EP_BLOCK / 64], s_tot[RC_EP_BLOCK / 64], s_wave[RC_EP_BLOCK / 64];
    const int A = d.cars_per_env;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // envs that log in the workgroups before this one, and in all of them
    uint32_t pre = 0, tot = 0;
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += RC_EP_BLOCK) {
        const uint32_t c = d.block_counts[i];
        tot += c;
        pre += i < blockIdx.x ? c : 0u;
    }
    pre = wave_sum(pre);
    tot = wave_sum(tot);
    const int e = blockIdx.x * RC_EP_BLOCK + threadIdx.x;
    const bool valid = e < d.num_envs;
    const bool act = valid && d.active[e] != 0;
    const bool ended = valid && ep_any_done(d, e);
    const uint32_t ordinal = valid ? d.ordinal[e] : 0u;
    const bool in_quota = d.max_episodes == 0u || ordinal < d.max_episodes;
    const bool logs = act && ended && in_quota;                // = ep_logs(d, e): nothing it reads has been written yet
    const bool skips = act && ended && !in_quota;
    const bool fills = act && ended && d.max_episodes != 0u && ordinal + 1u == d.max_episodes;
    const unsigned long long b_logs = __ballot(logs), b_skips = __ballot(skips), b_fills = __ballot(fills);
    if (lane == 0u) {
        s_pre[wave] = pre;
        s_tot[wave] = tot;
        s_wave[wave] = (uint32_t)__popcll(b_logs);
        if (b_skips) atomicAdd(&d.counters[RC_EPC_SKIPPED], (unsigned long long)__popcll(b_skips) * (unsigned long long)A);
        if (b_fills) atomicAdd(&d.counters[RC_EPC_AT_QUOTA], (unsigned long long)__popcll(b_fills));
    }
    __syncthreads();
    pre = tot = 0;
    uint32_t rank = lanes_below(b_logs);
#pragma unroll
    for (uint32_t w = 0; w < RC_EP_BLOCK / 64; ++w) {
        pre += s_pre[w];
        tot += s_tot[w];
        rank += w < wave ? s_wave[w] : 0u;
    }
    const unsigned long long cursor = d.cursor[d.call & 1u];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long asked = cursor + (unsigned long long)tot * (unsigned long long)A;
        const unsigned long long written = asked < d.capacity ? asked : d.capacity;
        d.cursor[(d.call + 1u) & 1u] = asked;
        d.counters[RC_EPC_WRITTEN] = written;
        d.counters[RC_EPC_DROPPED] = asked - written;
        d.counters[RC_EPC_CALLS] = (unsigned long long)d.call + 1ull;
    }
    if (!valid) return;
    if (act) {
        const int length = d.length[e] + 1;
        const unsigned long long at = cursor + (unsigned long long)(pre + rank) * (unsigned long long)A;
        for (int a = 0; a < A; ++a) {
            const int i = e * A + a;
            const float ret = d.ret[i] + d.reward[i];
            const float prog = fmaxf(d.prog_max[i], d.progress_total[i]);
            const float time = fmaxf(d.time_max[i], d.time[i]);
            const uint8_t wrong = d.wrong_seen[i] | (d.wrong[i] != 0 ? 1 : 0);
            if (!ended) {
                d.ret[i] = ret;
                d.prog_max[i] = prog;
                d.time_max[i] = time;
                d.wrong_seen[i] = wrong;
            } else if (logs && at + (unsigned long long)a < d.capacity) {
                RcEpisodeRow r;
                r.env = (int32_t)(d.first_env + (uint32_t)e);
                r.slot = a;
                r.track = d.track[e];
                r.episode = ordinal;
                r.call = d.call;
                r.length = length;
                r.ret = ret;
                r.progress = prog;
                r.time = time;
                r.laps = d.lap[i] - 1;
                r.flags = (d.wall[i] ? 1u : 0u) | (d.opp[i] ? 2u : 0u) | (d.trunc[i] ? 4u : 0u) | (wrong ? 8u : 0u) | (d.done[i] ? 16u : 0u);
                r.reserved = 0u;
                d.rows[at + (unsigned long long)a] = r;
            }
        }
        if (!ended) d.length[e] = length;
        else d.ordinal[e] = ordinal + 1u;
    }
    if (ended) {
        // respawned inside this call (auto-reset): the next episode runs from here, on the track the env has now; else the
        // env is frozen until rc_reset, and nothing more is summed or logged for it
        if (d.fresh[e * A] != 0) ep_start(d, e);
        else d.active[e] = 0;
    }
}

__global__ __launch_bounds__(RC_EP_BLOCK) void rc_episode_reset_kernel(RcEpisodeDev d, const uint8_t *__restrict__ mask) {
    const int e = blockIdx.x * RC_EP_BLOCK + threadIdx.x;
    const bool sel = e < d.num_envs && (mask == nullptr || mask[e] != 0);
    const unsigned long long b = __ballot(sel && d.active[e] != 0);      // a running episode ends here without a row
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&d.counters[RC_EPC_ABANDONED], (unsigned long long)__popcll(b));
    if (sel) ep_start(d, e);
}

}  // namespace

hipError_t rck_launch_episode_step(const RcEpisodeDev &d, hipStream_t s) {
    const int blocks = (d.num_envs + RC_EP_BLOCK - 1) / RC_EP_BLOCK;
    hipLaunchKernelGGL(rc_episode_count_kernel, dim3(blocks), dim3(RC_EP_BLOCK), 0, s, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rc_episode_update_kernel, dim3(blocks), dim3(RC_EP_BLOCK), 0, s, d);
    return hipGetLastError();
}

hipError_t rck_launch_episode_reset(const RcEpisodeDev &d, const uint8_t *mask_dev, hipStream_t s) {
    const int blocks = (d.num_envs + RC_EP_BLOCK - 1) / RC_EP_BLOCK;
    hipLaunchKernelGGL(rc_episode_reset_kernel, dim3(blocks), dim3(RC_EP_BLOCK), 0, s, d, mask_dev);
    return hipGetLastError();
}

// ---- the launches behind a step's dynamics and a reset, and the entry points (include/racecar_hip.h, rc_episode_log_*)
// The log reads the arena the outputs point at NOW (rc_set_arena re-points them between steps) and the current track ids.
void episode_bind(rc_env *env) {
    RcEpisodeDev &d = env->ep;
    const RcOutDev &o = env->params.out;
    d.reward = o.reward; d.progress_total = o.progress_total; d.time = o.time; d.lap = o.lap;
    d.done = o.done; d.trunc = o.trunc; d.wall = o.wall; d.opp = o.opp; d.wrong = o.wrong; d.fresh = o.fresh;
    d.ts_n = env->params.ts_n;
    d.ts_track = env->params.ts_n > 0 ? env->params.ts_track : nullptr;
    d.call = (uint32_t)env->ep_calls;
}

// After the dynamics launch and before the scan: the few fields the log reads are the ones that launch has just written (they
// are still in L2; behind the scan's 280 MB of rows they would not be), and the scan does not depend on the log.
int episode_step(rc_env *env) {
    episode_bind(env);
    KernelTimer t;
    int rc = t.begin(env, kTimeEpisodeLog, true);
    if (rc) return rc;
    HIP_TRY(rck_launch_episode_step(env->ep, env->stream));
    if ((rc = t.end())) return rc;
    env->ep_calls += 1;
    return RC_OK;
}

extern "C" {

static_assert(sizeof(rc_episode_row) == 48 && sizeof(RcEpisodeRow) == sizeof(rc_episode_row), "rc_episode_row is 48 bytes");

int rc_episode_log_enable(rc_env *env, int64_t capacity_rows, int32_t max_episodes) {
    if (capacity_rows < 1) return fail(RC_ERR_INVALID, "rc_episode_log_enable: capacity_rows must be >= 1 (got %lld)", (long long)capacity_rows);
    if (max_episodes < 0) return fail(RC_ERR_INVALID, "rc_episode_log_enable: max_episodes must be >= 0 (got %d)", max_episodes);
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    HIP_TRY(hipSetDevice(env->cfg.device));
    const size_t B = (size_t)env->cfg.num_envs, N = (size_t)env->n_cars, blocks = (B + RC_EP_BLOCK - 1) / RC_EP_BLOCK;
    RcEpisodeDev &d = env->ep;
    if (!env->ep_mem) {
        // counters [8] | cursor [2] | ordinal, length, track [B] | ret, prog_max, time_max [N] | block counts | active [B] | wrong_seen [N]
        const size_t bytes = 10 * 8 + 3 * B * 4 + 3 * N * 4 + blocks * 4 + B + N;
        HIP_TRY(hipMalloc(&env->ep_mem, bytes));
        HIP_TRY(hipMemsetAsync(env->ep_mem, 0, bytes, env->stream));      // active = 0: every env starts counting at its next reset
        d = RcEpisodeDev{};
        d.counters = (unsigned long long *)env->ep_mem;
        d.cursor = d.counters + 8;
        d.ordinal = (uint32_t *)(d.cursor + 2);
        d.length = (int32_t *)(d.ordinal + B);
        d.track = d.length + B;
        d.ret = (float *)(d.track + B);
        d.prog_max = d.ret + N;
        d.time_max = d.prog_max + N;
        d.block_counts = (uint32_t *)(d.time_max + N);
        d.active = (uint8_t *)(d.block_counts + blocks);
        d.wrong_seen = d.active + B;
        d.num_envs = env->cfg.num_envs;
        d.cars_per_env = env->cfg.cars_per_env;
        d.first_env = (uint32_t)env->cfg.first_env;
    }
    if (!env->ep_rows || d.capacity != (unsigned long long)capacity_rows) {
        if (env->ep_rows) {
            HIP_TRY(hipStreamSynchronize(env->stream));       // (launches that write the old rows may still be queued)
            HIP_TRY(hipFree(env->ep_rows));
            env->ep_rows = nullptr;
            env->ep_on = false;
        }
        if (hipMalloc(&env->ep_rows, (size_t)capacity_rows * sizeof(RcEpisodeRow)) != hipSuccess) {
            env->ep_rows = nullptr;
            return fail(RC_ERR_NOMEM, "rc_episode_log_enable: no device memory for %lld rows", (long long)capacity_rows);
        }
        d.rows = (RcEpisodeRow *)env->ep_rows;
        d.capacity = (unsigned long long)capacity_rows;
    }
    d.max_episodes = (uint32_t)max_episodes;
    env->ep_on = true;
    return rc_episode_log_clear(env);
}

int rc_episode_log_disable(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->ep_mem) return RC_OK;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    HIP_TRY(hipFree(env->ep_mem));
    env->ep_mem = nullptr;
    if (env->ep_rows) HIP_TRY(hipFree(env->ep_rows));
    env->ep_rows = nullptr;
    env->ep_on = false;
    env->ep = RcEpisodeDev{};
    return RC_OK;
}

int rc_episode_log(rc_env *env, void **rows_dev, size_t *capacity_rows, void **counters_dev, size_t *counters_bytes) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->ep_on) return fail(RC_ERR_INVALID, "rc_episode_log: the episode log is not enabled (rc_episode_log_enable)");
    if (rows_dev) *rows_dev = env->ep_rows;
    if (capacity_rows) *capacity_rows = (size_t)env->ep.capacity;
    if (counters_dev) *counters_dev = env->ep.counters;
    if (counters_bytes) *counters_bytes = RC_EPC_COUNT * sizeof(uint64_t);
    return RC_OK;
}

int rc_episode_log_clear(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->ep_on) return fail(RC_ERR_INVALID, "rc_episode_log_clear: the episode log is not enabled (rc_episode_log_enable)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    const RcEpisodeDev &d = env->ep;
    HIP_TRY(hipMemsetAsync(d.rows, 0, (size_t)d.capacity * sizeof(RcEpisodeRow), env->stream));
    HIP_TRY(hipMemsetAsync(d.counters, 0, 10 * 8, env->stream));                                  // the counters and the cursor pair
    HIP_TRY(hipMemsetAsync(d.ordinal, 0, (size_t)env->cfg.num_envs * 4, env->stream));
    env->ep_calls = 0;
    return RC_OK;
}

int rc_episode_log_time(rc_env *env, double *total_ms, uint64_t *launches) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    int rc = drain_events(env);
    if (rc) return rc;
    if (total_ms) *total_ms = env->k_ms[kTimeEpisodeLog];
    if (launches) *launches = env->k_n[kTimeEpisodeLog];
    return RC_OK;
}

}  // extern "C"
