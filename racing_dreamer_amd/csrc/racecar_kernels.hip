// HIP kernels of the batched racecar environment for MI355X (gfx950, wave64).
//
//   rc_dynamics_kernel  one lane per env: action remap, bicycle integrator (H2), wall / car-car
//                       collision (H5), progress + lap state machine, reward, done (H4, H15),
//                       in-kernel action repeat (H9), time limit (H10), auto-reset (H6)
//   rc_raycast_car_kernel  the LiDAR scan (H3), inter-car returns (H18): one wave per car, 17 rounds of 64 beams;
//                       exact grid traversal that crosses certified-free rectangles in one trip - the first from
//                       the per-cell first-trip table (by quadrant and slope bin), the later ones from the four
//                       quadrant planes; ranges staged in LDS and flushed at the end of the wave
//                       (device code: racecar_scan.h; the earlier forms of the scan, variants 0-6, and the instrumented
//                       build are NOT in this library: racecar_lab.hip, built on request, loaded on first use)
//   rc_build_quad_kernel, rc_build_first_kernel  build the quadrant planes and the first-trip table on the device
//                       at rc_load_track
//   rc_patch_car_kernel lidar_occupancy 64x64 ego patch (H11), one wave per car, drivable bitmap staged in LDS
//   rc_reset_kernel     masked reset from the centerline spawn table with Philox4x32-10 (H6)
//
// Numerics: fp32, one IEEE operation per written operator (-ffp-contract=off), same order as
// oracle/racecar_oracle.py, so results are bit-identical to the CPU oracle.
#include <dlfcn.h>
#include <initializer_list>
#include <mutex>
#include <string>

#include "racecar_scan.h"      // the traversal and scan_car (shared with the lab library, racecar_lab.hip)
#include "racecar_car.h"          // Car, wall_hit, obb_overlap (shared with the spawn-table builder, racecar_tracks.hip)
#include "racecar_step.h"         // load_cars, the env's track in a track set, controls_of, the sub-step's body (shared with the look-ahead, racecar_lookahead.hip)
#include "racecar_patch_exact.h"   // obs_type lidar_occupancy_reference

#define RC_PATCH 64

namespace {

// What rc_patch_car_kernel needs of a car (RcStateDev::patch_pose): the start cell, the pixel step of the 64 x 64 patch in
// 16.16 cells (heading = + column, 3.125 cells per pixel) - or the mark of an all-zero patch: the first observation of an
// episode (dreamer/wrappers.py:413) and a car tens of thousands of cells off the grid (a diverged state sees nothing; it also
// keeps the fixed-point taps in range).  Computed by whoever writes the pose (one lane per car), so that the render, one wave
// per car, starts from ONE scalar 16-byte load and spends no vector instruction on wave-uniform values.
__device__ __forceinline__ int4 patch_pose_of(const RcTrackDev &t, float x, float y, float ct, float st, int fresh) {
    int icx, icy;
    cell_of(t, x, y, icx, icy);
    icy += 1;
    const bool sane = (unsigned)(icx + 16384) < 32768u && (unsigned)(icy + 16384) < 32768u;
    const int a = (int)__builtin_rintf(ct * RCS_PATCH_STEP_Q16), b = (int)__builtin_rintf(st * RCS_PATCH_STEP_Q16);
    return make_int4((fresh != 0 || !sane) ? RC_PATCH_SKIP : icx, icy, a, b);
}

// Reset of one env in two halves.  `prepare_reset` is everything that does not depend on how the current step ends -
// the Philox draw keyed by (global env id, episode counter), the gather of the spawn poses and, in the random modes, the
// progress value at the jittered pose - so the dynamics kernel calls it ahead of the integrator, behind the state loads,
// instead of behind the step.  What the compiled kernel does with that: only the episode counter travels with the state; the
// chain episode -> Philox -> spawn gather -> jitter -> progress_at is then waited out IN FRONT of the integration, three
// dependent round trips in series ahead of the step's own footprint and progress loads (the kernel runs one wave per SIMD:
// its duration is the length of that chain).  The listing is in profiles/step_entry_isa.txt; a reordering that covers the
// gather and the progress load with the first sub-step's loads was built and measured and gained nothing that the headline
// shows (EXPERIMENTS.md 0000.3, tools/experiments/step_entry_dynamics.patch).  `apply_reset` installs the prepared poses
// when the env did finish.
struct Spawn { float x, y, th, ct, st, pr; int cp; };

__device__ __forceinline__ float unit_pm1(uint32_t w) { return ((float)(w >> 8) * 5.9604644775390625e-8f) * 2.0f - 1.0f; }   // [-1, 1), exact

__device__ __forceinline__ int obb_overlap_spawn(const Spawn &a, const Spawn &b) {
    Car ca, cb;
    ca.x = a.x; ca.y = a.y; ca.ct = a.ct; ca.st = a.st;
    cb.x = b.x; cb.y = b.y; cb.ct = b.ct; cb.st = b.st;
    return obb_overlap(ca, cb);
}

// The reset law (H6; oracle: _reset_envs).  `grid`: the cars on the centre line behind the start.  `random` / `random_ball`:
// word 0 of Philox(global env id, episode, 0, 0) picks a centre-line bin uniformly over the lap; car a stands at bin
// idx0 - a * BALL_GAP (row of the spawn table), moved sideways by u * w (w: the row's lateral room) and turned by v * h (h: its
// heading room, RCS_HEADING_JITTER wherever w > 0) off the track's direction; (u, v) = words 1, 2 of call 0 for car 0, words (0, 1) / (2, 3) of call 1 + (a - 1) / 2 for the others.
// If two proposed cars overlap, ALL cars of the env take the centre-line poses.
template <int A>
__device__ __forceinline__ void prepare_reset(const RcParams &p, const RcTrackDev &t, int e, uint32_t ep, Spawn (&sp)[A]) {
    const uint32_t g = p.first_env + (uint32_t)e;
    const bool jitter = p.reset_mode != 0;
    rcd::u32x4 r[1 + A / 2];
    r[0] = rcd::philox4x32(g, ep, 0u, 0u, p.seed_lo, p.seed_hi);
    if (jitter) {
#pragma unroll
        for (int k = 1; k < 1 + A / 2; ++k) r[k] = rcd::philox4x32(g, ep, (uint32_t)k, 0u, p.seed_lo, p.seed_hi);
    }
    const int n = t.n_centerline;
    int idx0 = !jitter ? RCS_BALL_GAP_BINS * (A - 1) + RCS_GRID_LEAD_BINS : (int)__umulhi(r[0].x, (uint32_t)n);
    if (A > 1) idx0 = __float_as_int(t.spawn[2 * idx0 + 1].z) >> 8;      // never anchor several cars where the centre line folds (the grid too)
    Spawn centre[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        int idx = (idx0 - a * RCS_BALL_GAP_BINS) % n;
        if (idx < 0) idx += n;
        const float4 s0 = t.spawn[2 * idx], s1 = t.spawn[2 * idx + 1];
        Spawn &c = centre[a];
        c.x = s0.x; c.y = s0.y; c.th = s0.z; c.ct = s0.w;
        c.st = s1.x; c.pr = s1.y; c.cp = __float_as_int(s1.z) & 0xff;
        sp[a] = c;
        if (jitter) {
            const rcd::u32x4 &q = r[a == 0 ? 0 : 1 + (a - 1) / 2];
            const uint32_t wu = a == 0 ? q.y : (((a - 1) & 1) ? q.z : q.x);
            const uint32_t wv = a == 0 ? q.z : (((a - 1) & 1) ? q.w : q.y);
            const float room = s1.w;                     // w > 0: lateral room, any heading; else - (heading room), no lateral room
            const float off = unit_pm1(wu) * fmaxf(room, 0.0f);
            Spawn &j = sp[a];
            j.x = c.x - off * c.st;
            j.y = c.y + off * c.ct;
            float th = c.th + unit_pm1(wv) * (room > 0.0f ? RCS_HEADING_JITTER : -room);
            th = th > RCS_PI ? th - RCS_TWO_PI : th;
            th = th < -RCS_PI ? th + RCS_TWO_PI : th;
            j.th = th;
            sincos32(th, j.st, j.ct);
            float pr = progress_at(t, j.x, j.y);
            pr = pr < 0.0f ? 0.0f : pr;
            j.pr = pr;
            const int cp = (int)(pr * (float)RCS_N_CHECKPOINTS);
            j.cp = cp < RCS_N_CHECKPOINTS - 1 ? cp : RCS_N_CHECKPOINTS - 1;
        }
    }
    if (A > 1 && jitter) {
        int clash = 0;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int b = a + 1; b < A; ++b) clash |= obb_overlap_spawn(sp[a], sp[b]);
        if (clash) {
#pragma unroll
            for (int a = 0; a < A; ++a) sp[a] = centre[a];
        }
    }
}

template <int A>
__device__ __forceinline__ void apply_reset(const RcParams &p, int e, Car (&car)[A], const Spawn (&sp)[A], uint32_t ep,
                                            int &steps, int &agent_steps) {
    p.st.episode[e] = ep + 1u;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        Car &c = car[a];
        c.x = sp[a].x; c.y = sp[a].y; c.th = sp[a].th; c.ct = sp[a].ct; c.st = sp[a].st;
        c.pr = sp[a].pr; c.cp = sp[a].cp;
        c.v = c.dl = c.om = c.ac = 0.0f;
        c.wall = c.opp = c.wrong = c.done = c.trunc = 0;
        c.lap = 1;
        c.fresh = 1;
        if (p.car_task[a] == 2) {                 // n_step_progress: the window starts at the spawn progress
            float *h = p.st.nstep_hist + (size_t)(e * A + a) * RC_NSTEP_MAX;
            for (int k = 0; k < RC_NSTEP_MAX; ++k) h[k] = sp[a].pr;
        }
    }
    steps = 0;
    agent_steps = 0;
}

// Vehicle randomization (rc_set_vehicle_randomization): the parameters of the cars of env e for the episode that a reset with
// episode value ep starts.  Word j = 5 a + i (car a, parameter i) is word j % 4 of Philox(global env id, ep, j / 4, RC_VP_TAG);
// value = lo + u (hi - lo), u = (w >> 8) 2^-24, one rounding per operator (lo == hi gives lo exactly).
template <int A>
__device__ __forceinline__ void draw_vehicle(const RcParams &p, int e, uint32_t ep, float (&vp)[A][RC_VP_COUNT]) {
    const uint32_t g = p.first_env + (uint32_t)e;
    constexpr int kCalls = (RC_VP_COUNT * A + 3) / 4;
    uint32_t w[4 * kCalls];
#pragma unroll
    for (int k = 0; k < kCalls; ++k) {
        const rcd::u32x4 r = rcd::philox4x32(g, ep, (uint32_t)k, RC_VP_TAG, p.vp_seed_lo, p.vp_seed_hi);
        w[4 * k] = r.x; w[4 * k + 1] = r.y; w[4 * k + 2] = r.z; w[4 * k + 3] = r.w;
    }
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int i = 0; i < RC_VP_COUNT; ++i) {
            const float u = (float)(w[RC_VP_COUNT * a + i] >> 8) * 5.9604644775390625e-8f;
            vp[a][i] = p.vp_lo[i] + u * (p.vp_hi[i] - p.vp_lo[i]);
        }
}

template <int A>
__device__ __forceinline__ void store_vehicle(const RcParams &p, int e, const float (&vp)[A][RC_VP_COUNT]) {
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int i = 0; i < RC_VP_COUNT; ++i) p.vparams[(size_t)(e * A + a) * RC_VP_COUNT + i] = vp[a][i];
}

template <int A>
__device__ __forceinline__ void store_state_and_obs(const RcParams &p, const RcTrackDev &t, int e, const Car (&car)[A], int steps,
                                                    int agent_steps) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        const Car &c = car[a];
        p.st.x[i] = c.x; p.st.y[i] = c.y; p.st.theta[i] = c.th; p.st.ct[i] = c.ct; p.st.st[i] = c.st;
        p.st.v[i] = c.v; p.st.delta[i] = c.dl; p.st.omega[i] = c.om; p.st.accel[i] = c.ac;
        p.st.progress[i] = c.pr; p.st.lap[i] = c.lap; p.st.cp[i] = c.cp;
        p.st.wall[i] = c.wall; p.st.opp[i] = c.opp; p.st.wrong[i] = c.wrong;
        p.st.done[i] = c.done; p.st.trunc[i] = c.trunc; p.st.fresh[i] = c.fresh;
        p.st.scan_pose[i] = make_float4(c.x, c.y, c.ct, c.st);
        if (p.render_patch) p.st.patch_pose[i] = patch_pose_of(t, c.x, c.y, c.ct, c.st, c.fresh);
        // observation of the current state (post auto-reset)
        float *pose = p.out.pose + 6 * i, *vel = p.out.velocity + 6 * i;
        pose[0] = c.x; pose[1] = c.y; pose[2] = 0.0f; pose[3] = 0.0f; pose[4] = 0.0f; pose[5] = c.th;
        vel[0] = c.v; vel[1] = 0.0f; vel[2] = 0.0f; vel[3] = 0.0f; vel[4] = 0.0f; vel[5] = c.om;
        p.out.speed[i] = fabsf(c.v);
        p.out.accel[i] = c.ac;
        p.out.steer[i] = c.dl;
        p.out.fresh[i] = c.fresh;
    }
    p.st.steps[e] = steps;
    p.st.agent_steps[e] = agent_steps;
}

// Results of the step that just ran (terminal values when the env finished).
template <int A>
__device__ __forceinline__ void store_step_results(const RcParams &p, int e, const Car (&car)[A], int steps) {
    const float time = (float)steps * RCS_DT;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        const Car &c = car[a];
        p.out.reward[i] = c.rew;
        p.out.discount[i] = 1.0f - (float)c.done;
        p.out.progress_total[i] = (float)(c.lap - 1) + c.pr;
        p.out.time[i] = time;
        p.out.progress[i] = c.pr;
        p.out.lap[i] = c.lap;
        p.out.cp[i] = c.cp;
        p.out.done[i] = c.done;
        p.out.trunc[i] = c.trunc;
        p.out.wall[i] = c.wall;
        p.out.opp[i] = c.opp;
        p.out.wrong[i] = c.wrong;
    }
}

// ---- track set (rc_set_track_set): ts_track_of and lane_track are in racecar_step.h
// The track of the episode that a reset with episode value ep starts (include/racecar_hip.h, rc_set_track_set): sequential
// k + 1 mod T; random word 0 of Philox(global env id, ep, 0, RC_TS_TAG) r, (r T) >> 32 or #{c_i <= r} with weights; manual
// next[e] (a value outside [0, T) keeps the current track).
__device__ __forceinline__ int ts_next_track(const RcParams &p, int e, uint32_t ep, int cur) {
    const int n = p.ts_n;
    if (p.ts_order == RC_TSO_SEQUENTIAL) return cur + 1 < n ? cur + 1 : 0;
    if (p.ts_order == RC_TSO_MANUAL) {
        const int k = p.ts_next[e];
        return (unsigned)k < (unsigned)n ? k : cur;
    }
    const uint32_t r = rcd::philox4x32(p.first_env + (uint32_t)e, ep, 0u, RC_TS_TAG, p.ts_seed_lo, p.ts_seed_hi).x;
    if (!p.ts_weighted) return (int)__umulhi(r, (uint32_t)n);
    int k = 0;
#pragma unroll
    for (int i = 0; i < RC_TS_MAX - 1; ++i) k += (i < n - 1 && p.ts_cum[i] <= r) ? 1 : 0;
    return k;
}

// ------------------------------------------------------------------------------------------------
template <int A, bool DR = false, bool TS = false>
// rand_on != 0: the actions are not read but drawn here, U(-1, 1)^2 from Philox keyed by (seed, step, global car id) -
// the same numbers rc_random_actions_kernel writes (synthetic random-action rollouts without a launch of their own);
// they are stored to `actions` as well, so the buffer shows what was applied.
// DR: the five vehicle parameters of the integrator come from the car (RcParams::vparams) instead of the spec's constants - the
// same operations in the same order, only the operand differs - and a reset in random mode draws them anew (draw_vehicle).
// TS: the env steps on its track (ts_track) and a reset starts on the next one (ts_next_track), drawn before the spawn.
__device__ __forceinline__ void dynamics_env(const RcParams &p, float *__restrict__ actions, const int repeat, const int rand_on,
                                             const uint32_t rand_lo, const uint32_t rand_hi, const uint32_t rand_step, const int e) {
    RcTrackDev tc_l = {}, tn_l = {};
    const RcTrackDev &t = TS ? tc_l : p.trk;
    const RcTrackDev &tn = TS ? tn_l : p.trk;
    // the episode counter first: it is the oldest load in flight, so the reset's Philox draw can wait for it alone
    const uint32_t episode = p.auto_reset ? p.st.episode[e] : 0u;
    int tr_next = 0;
    if (TS) {
        const int tr = ts_track_of(p, e);
        tr_next = (p.auto_reset && p.ts_started[e]) ? ts_next_track(p, e, episode, tr) : tr;
        lane_track(p, tr, tc_l);
        lane_track(p, tr_next, tn_l);
    }
    Car car[A];
    load_cars<A>(p, e, car);
    int steps = p.st.steps[e], agent_steps = p.st.agent_steps[e];
    Spawn spawn[A];
    if (p.auto_reset) prepare_reset<A>(p, tn, e, episode, spawn);      // ahead of the step: see prepare_reset
    float vp[A][RC_VP_COUNT];
    if (DR) {
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int i = 0; i < RC_VP_COUNT; ++i) vp[a][i] = p.vparams[(size_t)(e * A + a) * RC_VP_COUNT + i];
    }
    float motor[A], steer[A];
    bool any_done = false;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        float a0, a1;
        if (rand_on) {
            const rcd::u32x4 r = rcd::philox4x32(p.first_env * (uint32_t)A + (uint32_t)i, rand_step, 1u, 0u, rand_lo, rand_hi);
            a0 = (float)(r.x >> 8) * 5.9604644775390625e-8f * 2.0f - 1.0f;      // as rc_random_actions_kernel
            a1 = (float)(r.y >> 8) * 5.9604644775390625e-8f * 2.0f - 1.0f;
            actions[2 * i] = a0;
            actions[2 * i + 1] = a1;
        } else {
            a0 = actions[2 * i];
            a1 = actions[2 * i + 1];
        }
        p.out.action[2 * i] = a0;
        p.out.action[2 * i + 1] = a1;
        controls_of(p, a0, a1, motor[a], steer[a]);
        any_done |= car[a].done != 0;
    }

    if (!any_done) {
        for (int sub = 0; sub < repeat; ++sub) {   // ActionRepeat, dreamer/wrappers.py:107-116
#define RC_NSTEP_SLOT(a, k) (p.st.nstep_hist + (size_t)(e * A + a) * RC_NSTEP_MAX + (k))
#include "racecar_substep.inc"      // one sub-step: the text the look-ahead's dynamics_substep is made of (racecar_step.h)
#undef RC_NSTEP_SLOT
            if (stop) break;
        }
        agent_steps += 1;
        if (p.time_limit_steps > 0 && agent_steps >= p.time_limit_steps) {   // TimeLimit, wrappers.py:147-154
#pragma unroll
            for (int a = 0; a < A; ++a) { car[a].done = 1; car[a].trunc = 1; }
        }
    }
    store_step_results<A>(p, e, car, steps);
    if (p.auto_reset) {
        bool fin = false;
#pragma unroll
        for (int a = 0; a < A; ++a) fin |= car[a].done != 0;
        if (fin) {
            apply_reset<A>(p, e, car, spawn, episode, steps, agent_steps);
            if (DR && p.vp_mode == RC_VP_RANDOM) {
                draw_vehicle<A>(p, e, episode, vp);
                store_vehicle<A>(p, e, vp);
            }
            if (TS) {
                p.ts_track[e] = tr_next;
                p.ts_started[e] = 1;
                tc_l = tn_l;                                       // the observation is the new episode's, on its track
            }
        }
    }
    store_state_and_obs<A>(p, t, e, car, steps, agent_steps);
}

// The env of this lane (one lane per env); false: the lane is beyond the handle's envs and leaves.
__device__ __forceinline__ bool lane_env(const RcParams &p, int &e) {
    e = blockIdx.x * blockDim.x + threadIdx.x;
    return e < p.num_envs;
}

template <int A>
__global__ __launch_bounds__(256) void rc_dynamics_kernel(RcParams p, float *__restrict__ actions, int repeat,
                                                          int rand_on, uint32_t rand_lo, uint32_t rand_hi, uint32_t rand_step) {
    int e;
    if (lane_env(p, e)) dynamics_env<A>(p, actions, repeat, rand_on, rand_lo, rand_hi, rand_step, e);
}

// The same with the vehicle parameters per car (rc_set_vehicle_randomization / rc_set_vehicle_params): launched only while a
// handle's vp_mode is not off.
template <int A>
__global__ __launch_bounds__(256) void rc_dynamics_dr_kernel(RcParams p, float *__restrict__ actions, int repeat,
                                                             int rand_on, uint32_t rand_lo, uint32_t rand_hi, uint32_t rand_step) {
    int e;
    if (lane_env(p, e)) dynamics_env<A, true>(p, actions, repeat, rand_on, rand_lo, rand_hi, rand_step, e);
}

// The same with a track per env (rc_set_track_set): launched only while the handle's track set is on.
template <int A, bool DR>
__global__ __launch_bounds__(256) void rc_dynamics_ts_kernel(RcParams p, float *__restrict__ actions, int repeat,
                                                             int rand_on, uint32_t rand_lo, uint32_t rand_hi, uint32_t rand_step) {
    int e;
    if (lane_env(p, e)) dynamics_env<A, DR, true>(p, actions, repeat, rand_on, rand_lo, rand_hi, rand_step, e);
}

// Where the car of rank r (position along the track) stands in RcStateDev::order - see rc_order_place_kernel.
__device__ __forceinline__ uint32_t order_slot_of_rank(uint32_t r, uint32_t n) {
    const uint32_t whole = (n / (8u * RC_ORDER_REGION)) * (8u * RC_ORDER_REGION);
    if (r >= whole) return r;
    const uint32_t g = r / RC_ORDER_REGION, o = r % RC_ORDER_REGION;
    return ((g >> 3) * RC_ORDER_REGION + o) * 8u + (g & 7u);
}

// ---- Several handles in ONE launch (rc_step_group: one handle per track, each filling its block of cars of one arena).  A
// wave belongs to one block: it finds it among <= RC_GROUP_MAX wave ranges (scalar compares) and works from THAT block's
// RcParams, read from a device table with scalar loads - the same loads, from another address, that the single-handle
// kernels do from their argument block.  The device code is the single-handle kernels' (dynamics_env, scan_car).
__device__ __forceinline__ int group_block(const RcGroup &g, const int wave) {
    int b = 0;
#pragma unroll
    for (int k = 1; k < RC_GROUP_MAX; ++k) b += (k < g.n && wave >= g.wave_start[k]) ? 1 : 0;
    return b;
}

template <int A, bool DR>
__device__ __forceinline__ void dynamics_group_wave(const RcParams *__restrict__ params, const RcGroup &g, const int repeat, const int rand_on,
                                                    const uint32_t rand_lo, const uint32_t rand_hi, const uint32_t rand_step) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (wave >= g.wave_start[g.n]) return;
    const int b = group_block(g, wave);
    const RcParams p = params[b];           // a COPY (top-level pointer argument + uniform index: scalar loads; a reference would be
                                            // re-read after every store, the table not being known to stay as it is)
    const int e = (wave - g.wave_start[b]) * 64 + (int)(threadIdx.x & 63u);
    if (e >= p.num_envs) return;
    dynamics_env<A, DR>(p, g.actions[b], repeat, rand_on, rand_lo, rand_hi, rand_step, e);
}

template <int A>
__global__ __launch_bounds__(256) void rc_dynamics_group_kernel(const RcParams *__restrict__ params, RcGroup g, int repeat, int rand_on,
                                                                uint32_t rand_lo, uint32_t rand_hi, uint32_t rand_step) {
    dynamics_group_wave<A, false>(params, g, repeat, rand_on, rand_lo, rand_hi, rand_step);
}

// (a group in which some handle's vehicle parameters are per car; a block whose handle has them off reads its nominal values)
template <int A>
__global__ __launch_bounds__(256) void rc_dynamics_dr_group_kernel(const RcParams *__restrict__ params, RcGroup g, int repeat, int rand_on,
                                                                   uint32_t rand_lo, uint32_t rand_hi, uint32_t rand_step) {
    dynamics_group_wave<A, true>(params, g, repeat, rand_on, rand_lo, rand_hi, rand_step);
}

template <int A>
__device__ __forceinline__ void reset_env(const RcParams &p, const RcTrackDev &t, int e, uint32_t episode) {
    Car car[A];
    int steps, agent_steps;
#pragma unroll
    for (int a = 0; a < A; ++a) car[a].rew = 0.0f;
    Spawn spawn[A];
    prepare_reset<A>(p, t, e, episode, spawn);
    apply_reset<A>(p, e, car, spawn, episode, steps, agent_steps);
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        p.out.action[2 * i] = 0.0f;       // Collect.reset, dreamer/wrappers.py:232
        p.out.action[2 * i + 1] = 0.0f;
    }
    store_step_results<A>(p, e, car, steps);
    store_state_and_obs<A>(p, t, e, car, steps, agent_steps);
}

// rc_reset's mask: an env that keeps running is left as it is
__device__ __forceinline__ bool masked_out(const uint8_t *__restrict__ mask, int e) { return mask != nullptr && mask[e] == 0; }

template <int A>
__global__ __launch_bounds__(256) void rc_reset_kernel(RcParams p, const uint8_t *__restrict__ mask) {
    int e;
    if (!lane_env(p, e) || masked_out(mask, e)) return;
    const uint32_t episode = p.st.episode[e];
    reset_env<A>(p, p.trk, e, episode);
}

// rc_reset with a track set: the env's next track first (its first reset after the install keeps the initial one), then the
// reset above on that track
template <int A>
__global__ __launch_bounds__(256) void rc_reset_ts_kernel(RcParams p, const uint8_t *__restrict__ mask) {
    int e;
    if (!lane_env(p, e) || masked_out(mask, e)) return;
    const uint32_t episode = p.st.episode[e];
    const int tr = ts_track_of(p, e);
    const int tr_next = p.ts_started[e] ? ts_next_track(p, e, episode, tr) : tr;
    RcTrackDev t = {};
    lane_track(p, tr_next, t);
    reset_env<A>(p, t, e, episode);
    p.ts_track[e] = tr_next;
    p.ts_started[e] = 1;
}

// rc_reset with vehicle randomization in random mode: the reset above, then the new episode's vehicle parameters
template <int A>
__global__ __launch_bounds__(256) void rc_reset_dr_kernel(RcParams p, const uint8_t *__restrict__ mask) {
    int e;
    if (!lane_env(p, e) || masked_out(mask, e)) return;
    const uint32_t episode = p.st.episode[e];
    float vp[A][RC_VP_COUNT];
    draw_vehicle<A>(p, e, episode, vp);
    store_vehicle<A>(p, e, vp);
}

// Device self-test of that property (rc_selftest_reciprocal): every fp32 with biased exponent in [exp_lo, exp_hi],
// both signs, fast path against IEEE division.
__global__ __launch_bounds__(256) void rc_selftest_rcp_kernel(uint32_t exp_lo, uint32_t exp_hi,
                                                              unsigned long long *mismatches) {
    const uint64_t total = (uint64_t)(exp_hi - exp_lo + 1) << 23;
    unsigned long long bad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = ((exp_lo + (uint32_t)(i >> 23)) << 23) | (uint32_t)(i & 0x7fffffu);
        const float d = __uint_as_float(bits), one = 1.0f;
        const float rp = __builtin_amdgcn_rcpf(d), rn = __builtin_amdgcn_rcpf(-d);          // the fast path of ray_reciprocals
        const float fx = __builtin_fmaf(__builtin_fmaf(-d, rp, 1.0f), rp, rp), fy = __builtin_fmaf(__builtin_fmaf(d, rn, 1.0f), rn, rn);
        bad += __float_as_uint(fx) != __float_as_uint(one / d);
        bad += __float_as_uint(fy) != __float_as_uint(one / -d);
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Variant 7: the traversal of variant 6 with ONE WAVE PER CAR.  The car index is wave-uniform, so the car state
// comes through scalar loads, everything that depends only on the car (sensor position, start cell, its range
// test) is computed once instead of once per 64 beams, and the wave walks its car's 1080 beams in 17 rounds of
// 64 (the last with 56 active lanes) - consecutive rounds start from the same cell, so their table lines are
// still in L1.  No persistent loop: 65 536 independent waves are balanced by the hardware dispatcher, where
// equal shares of chunks per resident workgroup left the slowest workgroup's tail exposed.
// `split` waves share a car (wave part k takes rounds k, k + split, ...): small batches still fill the chip.
template <int A, bool OVERLAP, bool GUARD>
__global__ __launch_bounds__(256) void rc_raycast_car_kernel(RcParams p, int split) {
    // One car (or 1 / split of one) per wave and nothing more: several cars in sequence per wave were measured slower
    // (2 per wave + 6 %, 8 per wave + 20 %) - the hardware dispatcher balances 65 536 short waves better than any
    // static share, and a finished wave's flush is not waited for by anybody.
    constexpr bool kOne = scan_one_wave_per_car<false, OVERLAP, GUARD>();
    const unsigned zero = scan_args_at_entry<kOne>(p, split);
    const uint32_t lds_row = wave_lds_row();                             // 17 x 64 floats per wave of the workgroup
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) + zero;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned slot = kOne ? wave : wave / (unsigned)split, part = kOne ? 0u : wave - slot * (unsigned)split;
    if (slot >= (unsigned)p.n_cars) return;
    // (the waves take the cars in track order - see RcStateDev::order -: 5 % of the scan at 65 536 cars, EXPERIMENTS I.11)
    const unsigned car = p.st.order != nullptr ? (unsigned)p.st.order[slot] : slot;
    scan_car<A, false, OVERLAP, GUARD>(p, car, part, split, lane, lds_row);
}

template <int A, bool OVERLAP>
__global__ __launch_bounds__(256) void rc_raycast_group_kernel(const RcParams *__restrict__ params, RcGroup g, int split) {
    const uint32_t lds_row = wave_lds_row();
    // Workgroups go to the 8 XCDs in turn, each with an L2 of its own: workgroup i takes wave (i mod 8) x ceil(W / 8) + i / 8, so
    // that an XCD works through ONE stretch of the car order - one track's tables in its L2, two at a block boundary - instead
    // of every eighth car of all tracks.
    const int launched = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int per_xcd = (g.wave_start[g.n] + 7) >> 3;
    const int wave = (launched & 7) * per_xcd + (launched >> 3);
    if ((launched >> 3) >= per_xcd || wave >= g.wave_start[g.n]) return;
    const int b = group_block(g, wave);
    const RcParams p = params[b];           // (a copy: see dynamics_group_wave)
    constexpr bool kOne = scan_one_wave_per_car<false, OVERLAP, false>();
    const unsigned local = (unsigned)(wave - g.wave_start[b]) + scan_args_at_entry<kOne>(p, split);      // (here: one batch of loads from the table)
    const unsigned slot = kOne ? local : local / (unsigned)split, part = kOne ? 0u : local - slot * (unsigned)split;
    if (slot >= (unsigned)p.n_cars) return;
    // (this launch hands every XCD a STRETCH of the slots, not every eighth: it takes the cars by rank)
    const unsigned car = p.st.order != nullptr ? (unsigned)p.st.order[order_slot_of_rank(slot, (uint32_t)p.n_cars)] : slot;
    scan_car<A, false, OVERLAP, false>(p, car, part, split, threadIdx.x & 63u, lds_row);
}

// The scan with LiDAR noise and dropout (rc_set_lidar_noise; scan_car's NOISE, lidar_noise in racecar_scan.h): new
// instantiations, launched only while a handle's noise is on, so the production kernels above stay what they were.
template <int A, bool OVERLAP>
__global__ __launch_bounds__(256) void rc_raycast_car_noise_kernel(RcParams p, int split) {
    constexpr bool kOne = scan_one_wave_per_car<false, OVERLAP, false>();
    const unsigned zero = scan_args_at_entry<kOne>(p, split);
    const uint32_t lds_row = wave_lds_row();
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) + zero;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned slot = kOne ? wave : wave / (unsigned)split, part = kOne ? 0u : wave - slot * (unsigned)split;
    if (slot >= (unsigned)p.n_cars) return;
    const unsigned car = p.st.order != nullptr ? (unsigned)p.st.order[slot] : slot;
    scan_car<A, false, OVERLAP, false, true>(p, car, part, split, lane, lds_row);
}

template <int A, bool OVERLAP>
__global__ __launch_bounds__(256) void rc_raycast_group_noise_kernel(const RcParams *__restrict__ params, RcGroup g, int split) {
    const uint32_t lds_row = wave_lds_row();
    const int launched = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int per_xcd = (g.wave_start[g.n] + 7) >> 3;
    const int wave = (launched & 7) * per_xcd + (launched >> 3);
    if ((launched >> 3) >= per_xcd || wave >= g.wave_start[g.n]) return;
    const int b = group_block(g, wave);
    const RcParams p = params[b];
    constexpr bool kOne = scan_one_wave_per_car<false, OVERLAP, false>();
    const unsigned local = (unsigned)(wave - g.wave_start[b]) + scan_args_at_entry<kOne>(p, split);      // (here: one batch of loads from the table)
    const unsigned slot = kOne ? local : local / (unsigned)split, part = kOne ? 0u : local - slot * (unsigned)split;
    if (slot >= (unsigned)p.n_cars) return;
    const unsigned car = p.st.order != nullptr ? (unsigned)p.st.order[order_slot_of_rank(slot, (uint32_t)p.n_cars)] : slot;
    scan_car<A, false, OVERLAP, false, true>(p, car, part, split, threadIdx.x & 63u, lds_row);
}

// ---- track set (rc_set_track_set).  The cars track-major: ts_list = the cars grouped by their env's track, each track's cars in
// the progress order (RcStateDev::order, by rank; car index order without it) as far as the waves' arrival order keeps it (a
// matter of locality, not of results), ts_start = where each track begins.  Three small launches at every observation (tracks
// change at every episode end; the progress part follows the sort's RC_ORDER_PERIOD): a ballot per track and wave counts the cars
// (one atomic per track and wave), one wave turns the counts into starts and cursors (and clears the counts for the next
// observation), and every wave takes its places per track with one atomic and writes its cars.  ts_count = ts_start + RC_TS_MAX + 1,
// the cursors behind it.
__device__ __forceinline__ int ts_car_at(const RcParams &p, int r) {
    return p.st.order != nullptr ? p.st.order[order_slot_of_rank((uint32_t)r, (uint32_t)p.n_cars)] : r;
}

__global__ __launch_bounds__(256) void rc_ts_count_kernel(RcParams p) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = r < p.n_cars ? ts_track_of(p, ts_car_at(p, r) / p.cars_per_env) : -1;
    int32_t *count = p.ts_start + RC_TS_MAX + 1;
#pragma unroll
    for (int j = 0; j < RC_TS_MAX; ++j) {
        const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(k == j));
        if ((threadIdx.x & 63u) == 0 && c != 0) atomicAdd(count + j, c);
    }
}

__global__ __launch_bounds__(64) void rc_ts_start_kernel(RcParams p) {
    int32_t *count = p.ts_start + RC_TS_MAX + 1, *cursor = count + RC_TS_MAX;
    const int lane = (int)threadIdx.x;
    int c[RC_TS_MAX];
#pragma unroll
    for (int j = 0; j < RC_TS_MAX; ++j) c[j] = count[j];
    int start = 0;
#pragma unroll
    for (int j = 0; j < RC_TS_MAX; ++j) start += (j < lane && j < p.ts_n) ? c[j] : 0;
    if (lane <= RC_TS_MAX) p.ts_start[lane] = start;
    if (lane < RC_TS_MAX) {
        cursor[lane] = start;
        count[lane] = 0;
    }
}

__global__ __launch_bounds__(256) void rc_ts_place_kernel(RcParams p) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int car = r < p.n_cars ? ts_car_at(p, r) : 0;
    const int k = r < p.n_cars ? ts_track_of(p, car / p.cars_per_env) : -1;
    int32_t *cursor = p.ts_start + RC_TS_MAX + 1 + RC_TS_MAX;
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int j = 0; j < RC_TS_MAX; ++j) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(k == j);
        if (m == 0) continue;                                              // (wave-uniform)
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(cursor + j, __builtin_popcountll(m));
        base = __shfl(base, leader);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (k == j) p.ts_list[base + below] = car;
    }
}

// The scan with a track per car: one wave per car (or 1 / split of one) as rc_raycast_group_kernel, the car taken from ts_list
// (every XCD a stretch of it: one or two tracks' tables in its L2) and its parameters - the owner's with its track's tables - from
// the table by its env's track with scalar loads.  NOISE: scan_car's LiDAR noise.
template <int A, bool OVERLAP, bool NOISE>
__global__ __launch_bounds__(256) void rc_raycast_ts_kernel(RcParams p0, int split) {
    const uint32_t lds_row = wave_lds_row();
    const int launched = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int total = p0.n_cars * split;
    const int per_xcd = (total + 7) >> 3;
    const int wave = (launched & 7) * per_xcd + (launched >> 3);
    if ((launched >> 3) >= per_xcd || wave >= total) return;
    constexpr bool kOne = scan_one_wave_per_car<false, OVERLAP, false>();
    const unsigned slot = kOne ? (unsigned)wave : (unsigned)wave / (unsigned)split, part = kOne ? 0u : (unsigned)wave - slot * (unsigned)split;
    const unsigned car = (unsigned)__builtin_amdgcn_readfirstlane(p0.ts_list[slot]);
    const int k = __builtin_amdgcn_readfirstlane(ts_track_of(p0, (int)(car / (unsigned)A)));
    const RcParams p = p0.ts_table[k];      // (a copy: see dynamics_group_wave)
    const unsigned zero = scan_args_at_entry<kOne>(p, split);      // (here: one batch of loads from the table)
    scan_car<A, false, OVERLAP, false, NOISE>(p, car + zero, part, split, threadIdx.x & 63u, lds_row);
}

// lidar_occupancy (H11, dreamer/wrappers.py:390-408): ego-aligned 64x64 patch of the drivable area,
// heading = +col, 3.125 cells per pixel, 1 = drivable.  Direct inverse map of the reference's
// crop -> rotate -> centre-crop -> resize chain: centred on the north-west corner of the car's cell,
// one nearest-cell tap per pixel, taps outside the reference's 220-cell crop window read 0.
//
// Tap positions are the spec's 16.16 fixed-point walk (oracle/racecar_oracle.py, render_patch): with
// (a, b) = rne(3.125 * 65536 * (cos, sin)) pixel (row r, col c) taps cell offset (X >> 16, Y >> 16),
// X = X00 + c a + r b, Y = Y00 + c b - r a.  One lane renders 16 adjacent pixels of a row (a quarter row) and stores
// them as one 16-byte vector; per pixel that is two integer adds, and because the start cell is folded into X and Y the
// byte address of the tap in the LDS bitmap is one shift and one 16 x 16-bit multiply-add that reads Y's high half
// directly: add, add, shift, mad, bit index, LDS byte read, shift into the pixel's byte lane = 6 vector instructions per
// pixel (20 in the fp32 form this replaces).  The window / grid test is hoisted out of the pixel loop: the valid taps of a
// run lie in the rectangle window-intersected-with-grid, which is convex, so a run whose two end taps are valid
// is valid throughout - a wave whose 64 runs all pass that test takes the test-free loop; the others (runs that
// cross a rotated corner of the window) take the loop that tests every tap (11 per pixel).
__device__ __forceinline__ uint32_t bfe_u32(uint32_t v, uint32_t offset, uint32_t width) {       // offset, width mod 32
    uint32_t r;
    asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(offset), "v"(width));
    return r;
}
__device__ __forceinline__ int mad_i24(int a, int b, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

// (Round 4: every operand that used to be wave-uniform - the pixel step, the grid limits, the window - sits in a VECTOR
// register: on gfx950 a vector instruction with a scalar-register operand issues at half rate (4.3 cycles against 2.35,
// tools/ubench/valu_issue4.hip), and the render is bound by exactly that - profiles/r04_a_pmc_patch_kernel_round3_build.txt:
// 47.1 M wave-level vector instructions per 65 536 cars, 97.6 % lane use, 58 % of the wave-cycles spent waiting to issue;
// 4.85 LDS cycles per byte gather of which 2.8 are bank conflicts, but the LDS pipe is only 40 % busy.)
__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_min_u32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t mad_hi16_s(uint32_t y, uint32_t pitch, uint32_t c) {         // (y >> 16) * pitch + c, pitch scalar
    uint32_t r;
    asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(r) : "v"(y), "s"(pitch), "v"(c));
    return r;
}
// byte BYTE of acc = low byte of (v >> sh), the other bytes of acc kept: extraction and packing of a pixel in ONE instruction
// (sub-dword addressing writes the result into the byte lane; the bits above the wanted one are cleared once per word)
template <int BYTE>
__device__ __forceinline__ uint32_t shr_into_byte(uint32_t acc, uint32_t sh, uint32_t v) {
    if (BYTE == 0) {
        asm("v_lshrrev_b32 %0, %1, %2" : "=v"(acc) : "v"(sh), "v"(v));
    } else if (BYTE == 1) {
        asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(acc) : "v"(sh), "v"(v));
    } else if (BYTE == 2) {
        asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(acc) : "v"(sh), "v"(v));
    } else {
        asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(acc) : "v"(sh), "v"(v));
    }
    return acc;
}
template <int I>
__device__ __forceinline__ void patch_put(uint32_t (&words)[4], uint32_t sh, uint32_t v) {
    words[I >> 2] = shr_into_byte<I & 3>(words[I >> 2], sh, v);
}
struct PatchConst {          // per car, all in vector registers (see above)
    int a, b;                // pixel step
    uint32_t xmax, ymax;     // last cell of the grid, 16.16 + 0xffff
    uint32_t wx, wy, span;   // the reference's crop window: origin and extent - 1 ulp
    uint32_t zero_addr;      // LDS address of the all-zero word behind the bitmap
    uint32_t three, one;     // the widths of the two bit-field extracts
    uint32_t sixteen;
    uint32_t ones;           // 0x01010101: bit 0 of every pixel byte
};

// One 16-pixel run: taps (X, Y) += (a, b).  CLAMP: coordinates are forced into the grid first - a tap left of / below
// the grid has a negative coordinate, i.e. a huge unsigned one, and clamps like one beyond the far edge to the last
// column / row, which is never drivable (rc_load_track clears the bitmap's outermost ring; so does the oracle).
// Per pixel: add, add, shift, multiply-add, bit index, LDS byte read, shift-into-its-byte-lane (sub-dword addressing: the
// extract and the pack in one instruction), + one mask per word = 6.25 vector instructions.
template <bool CLAMP, bool TESTED, int I>
struct PatchStep {
    static __device__ __forceinline__ void run(const __attribute__((address_space(3))) uint8_t *lds, int X, int Y, const PatchConst &k,
                                               uint32_t pitch_b, uint32_t (&words)[4]) {
        const uint32_t xc = CLAMP ? min_u32((uint32_t)X, k.xmax) : (uint32_t)X;
        const uint32_t yc = CLAMP ? min_u32((uint32_t)Y, k.ymax) : (uint32_t)Y;
        uint32_t addr = mad_hi16_s(yc, pitch_b, xc >> 19);                        // iy * pitch + ix / 8
        if (TESTED) {
            // inside the window <=> both window-relative coordinates (unsigned: below the window = huge) are <= 220 cells - 1 ulp
            const uint32_t far = max((uint32_t)X - k.wx, (uint32_t)Y - k.wy);
            addr = far <= k.span ? addr : k.zero_addr;
        }
        const uint32_t byte = lds[addr];
        patch_put<I>(words, bfe_u32(xc, k.sixteen, k.three), byte);              // byte I & 3 of its word = byte >> (ix % 8)
        PatchStep<CLAMP, TESTED, I + 1>::run(lds, X + k.a, Y + k.b, k, pitch_b, words);
    }
};
template <bool CLAMP, bool TESTED>
struct PatchStep<CLAMP, TESTED, 16> {
    static __device__ __forceinline__ void run(const __attribute__((address_space(3))) uint8_t *, int, int, const PatchConst &k, uint32_t,
                                               uint32_t (&words)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) words[j] &= k.ones;                            // keep bit 0 of every byte
    }
};
template <bool CLAMP>
__device__ __forceinline__ void patch_run(const __attribute__((address_space(3))) uint8_t *lds, int X, int Y, const PatchConst &k,
                                          uint32_t pitch_b, uint32_t (&words)[4]) {
    PatchStep<CLAMP, false, 0>::run(lds, X, Y, k, pitch_b, words);
}

// The same with every tap tested against the crop window (the corner runs of a car whose window corner cuts them).
template <bool CLAMP>
__device__ __forceinline__ void patch_run_tested(const __attribute__((address_space(3))) uint8_t *lds, int X, int Y, const PatchConst &k,
                                                 uint32_t pitch_b, uint32_t (&words)[4]) {
    PatchStep<CLAMP, true, 0>::run(lds, X, Y, k, pitch_b, words);
}

// ---- lidar_occupancy, ONE WAVE PER CAR -----------------------------------------------------------------------------
// (Round 3 gave a car to one wave - EXPERIMENTS.md I.1; round 4 took the wave-uniform work out of the vector unit.)
// * the car arrives as ONE scalar 16-byte load of integers (RcStateDev::patch_pose, written by the kernel that moved the car):
//   start cell, pixel step, or the mark of an all-zero patch; the window tests, the tap of pixel (0, 0) and the store base are
//   scalar arithmetic; the vector unit only walks pixels;
// * a lane renders four runs of 16 pixels, one per 16-row group g, and a store instruction writes group g of every lane:
//   lanes 4 i .. 4 i + 3 hold the four pieces of row 16 g + i, so every store covers whole 64-byte lines (16 rows = 1 KB
//   of consecutive bytes) - no line is split between waves or between instructions (HBM writes = 1.00 x the pixels);
// * only the 64 runs in the corner blocks (rows 0-15 and 48-63, columns 0-15 and 48-63) can be cut by the reference's
//   220-cell crop window.  In group 0 they are the lanes with l & 3 in {0, 3}; group 3 stores its pieces in the order
//   1, 0, 3, 2 (column block (l & 3) ^ 1: still whole lines per instruction), so there they are the lanes with l & 3 in
//   {1, 2}: EVERY lane owns exactly one corner run and renders it in one slot - with the tested loop only if some corner
//   run of the wave is in fact cut (its two end taps outside the window, which is convex) - and its three other runs with
//   the test-free loop.  That those cannot be cut is a property of the pixel step alone: a tap of a run outside the corner
//   blocks lies at most 31.5 |a| + 15.5 |b| (or the same with a and b exchanged) from the start cell on either axis, and
//   the SCALAR unit checks that bound against the window per car (it holds for every unit heading: 35.1 x 3.125 = 109.7
//   < 110 cells); a car that failed it would take the tested loop in all four slots.
struct PatchImage {          // the bitmap as it lies in LDS (wave-uniform): plain, or with the zero border of RC_PATCH_PAD cells
    uint32_t pitch_b, w_cells, h_cells, zero_addr;
};
template <bool CLAMP, bool NT>
__device__ __forceinline__ void patch_car(const RcParams &p, const PatchImage &img, const unsigned car, const unsigned lane, const int icx,
                                          const int icy, const int a, const int b, const bool all_tested) {
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(3))) uint8_t *lds_u8_ptr;
    const lds_u8_ptr lds_bytes = (lds_u8_ptr)(uint32_t)0;                // the bitmap starts at LDS address 0 (rck_set_lds_limits)
    const uint32_t pitch_b = img.pitch_b;
    PatchConst k;
    k.a = pin_vgpr(a); k.b = pin_vgpr(b);
    k.xmax = pin_vgpr(((img.w_cells - 1u) << 16) | 0xffffu);
    k.ymax = pin_vgpr(((img.h_cells - 1u) << 16) | 0xffffu);
    k.zero_addr = pin_vgpr(img.zero_addr);                               // a word that reads 0
    // the reference's [-110, 110) crop window around the start cell, in 16.16
    k.wx = pin_vgpr((uint32_t)(icx - RCS_PATCH_WINDOW_I) << 16);
    k.wy = pin_vgpr((uint32_t)(icy - RCS_PATCH_WINDOW_I) << 16);
    k.span = pin_vgpr(((uint32_t)(2 * RCS_PATCH_WINDOW_I) << 16) - 1u);
    k.three = pin_vgpr(3u); k.one = pin_vgpr(1u); k.sixteen = pin_vgpr(16u);
    k.ones = pin_vgpr(0x01010101u);
    const int x00 = ((63 * (-a - b)) >> 1) + icx * 65536, y00 = ((63 * (a - b)) >> 1) + icy * 65536;      // scalar
    const int rl = (int)(lane >> 2), cb = (int)(lane & 3u);
    const bool corner_first = cb == 0 || cb == 3;          // this lane's corner run is in group 0 (else in group 3)
    // start taps of a run: (row, first column c0)
    auto start = [&](int row, int c0, int &X, int &Y) {
        X = mad_i24(c0, a, mad_i24(row, b, x00));
        Y = mad_i24(c0, b, mad_i24(-row, a, y00));
    };
    auto ends_inside = [&](int X, int Y) {
        const uint32_t f0 = max((uint32_t)X - k.wx, (uint32_t)Y - k.wy);
        const uint32_t f1 = max((uint32_t)(X + 15 * k.a) - k.wx, (uint32_t)(Y + 15 * k.b) - k.wy);
        return (uint32_t)max(f0, f1) <= k.span;
    };
    // CLAMP cars (the window is not wholly inside the grid): a slot whose 64 runs all have BOTH end taps inside the grid - a
    // rectangle, convex - has every tap inside it and takes the loop without the two clamps per pixel; the others clamp
    auto slot_in_grid = [&](int X, int Y) {
        if (!CLAMP) return true;
        const uint32_t fx = max((uint32_t)X, (uint32_t)(X + 15 * (int)k.a)), fy = max((uint32_t)Y, (uint32_t)(Y + 15 * (int)k.b));
        return __builtin_amdgcn_ballot_w64(fx > k.xmax || fy > k.ymax) == 0;
    };
    // piece (row, column block) of the car's 4 KB lies at 16-byte index 4 row + block: groups 0 - 2 at 64 g + lane, group 3
    // (pieces in the order 1, 0, 3, 2) at 192 + (lane ^ 1)
    v4u_t *out = reinterpret_cast<v4u_t *>(p.out.patch) + (size_t)car * 256u;
    auto store = [&](int g, const uint32_t (&w)[4]) {
        const v4u_t px = {w[0], w[1], w[2], w[3]};
        v4u_t *dst = out + 64 * g + (g == 3 ? (lane ^ 1u) : lane);
        if (NT) __builtin_nontemporal_store(px, dst);
        else *dst = px;
    };
    // slot A: the corner run - group 0 piece cb for the lanes with cb in {0, 3}, group 3 piece cb ^ 1 for the others
    uint32_t wa[4], wb[4];
    {
        int X, Y;
        start(corner_first ? rl : 48 + rl, corner_first ? 16 * cb : 16 * (cb ^ 1), X, Y);
        // the end taps of every corner run inside the window, which is convex: so is every tap of the wave
        if (!all_tested && __builtin_amdgcn_ballot_w64(!ends_inside(X, Y)) == 0) {
            if (slot_in_grid(X, Y)) patch_run<false>(lds_bytes, X, Y, k, pitch_b, wa);
            else patch_run<CLAMP>(lds_bytes, X, Y, k, pitch_b, wa);
        } else {
            patch_run_tested<CLAMP>(lds_bytes, X, Y, k, pitch_b, wa);
        }
    }
    // slot B: the lane's piece of the OTHER outer group (columns 16 - 47: never cut); then groups 1 and 2
#pragma unroll 1
    for (int s = 0; s < 3; ++s) {
        const int row = s == 0 ? (corner_first ? 48 + rl : rl) : 16 * s + rl;
        const int c0 = (s == 0 && corner_first) ? 16 * (cb ^ 1) : 16 * cb;
        int X, Y;
        start(row, c0, X, Y);
        uint32_t w[4];
        if (all_tested) patch_run_tested<CLAMP>(lds_bytes, X, Y, k, pitch_b, w);
        else if (slot_in_grid(X, Y)) patch_run<false>(lds_bytes, X, Y, k, pitch_b, w);
        else patch_run<CLAMP>(lds_bytes, X, Y, k, pitch_b, w);
        if (s == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) wb[i] = w[i];
        } else {
            store(s, w);
        }
    }
    // (selecting the ADDRESS instead of the data - one select per store, each instruction then writing half of group 0's and half of
    // group 3's lines - saves 33 instructions per car and gains nothing: 0.0707 against 0.0701 ms, HBM writes 1.018 x; round 4)
    uint32_t g0[4], g3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        g0[i] = corner_first ? wa[i] : wb[i];
        g3[i] = corner_first ? wb[i] : wa[i];
    }
    store(0, g0);
    store(3, g3);
}

template <bool NT>
__global__ __launch_bounds__(1024) void rc_patch_car_kernel(RcParams p, int padded_bytes) {
    extern __shared__ uint32_t lds_words[];
    const RcTrackDev &t = p.trk;
    const int pad = padded_bytes > 0 ? RC_PATCH_PAD : 0;
    PatchImage img;
    if (pad) {
        // the bitmap inside a border of `pad` zero cells (pad = 5 words: rows keep their word alignment)
        const int pw = (t.w + 2 * pad + 31) / 32, rows = t.h + 2 * pad;
        uint4 *d4 = reinterpret_cast<uint4 *>(lds_words);
        const uint4 z4 = {0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < (padded_bytes >> 4); i += blockDim.x) d4[i] = z4;
        __syncthreads();
        for (int i = threadIdx.x; i < t.h * t.pitch; i += blockDim.x) {
            const int row = i / t.pitch, word = i - row * t.pitch;
            if (word < pw - pad / 32) lds_words[(row + pad) * pw + pad / 32 + word] = t.drv_words[i];
        }
        img.pitch_b = (uint32_t)pw * 4u; img.w_cells = (uint32_t)(pw * 32); img.h_cells = (uint32_t)rows; img.zero_addr = 0u;
    } else {
        stage_bitmap(lds_words, t.drv_words, t.h * t.pitch + 1);        // + the all-zero word behind the bitmap (rc_load_track)
        img.pitch_b = (uint32_t)t.pitch * 4u; img.w_cells = (uint32_t)t.w; img.h_cells = (uint32_t)t.h;
        img.zero_addr = (uint32_t)(t.h * t.pitch) * 4u;
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    // cars are dealt to the waves of the grid in turn (a wave's cars are `waves` apart: neighbouring waves write
    // neighbouring patches).  The car is wave-uniform, so its header comes through the SCALAR unit: vector loads share one
    // in-order counter with the stores, and every car would start by waiting for the previous car's 4 KB to be
    // acknowledged.  (Inline assembly with its own wait: the compiler takes the load for a vector one because the kernel
    // also stores.)
    for (unsigned car = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); car < (unsigned)p.n_cars;
         car = __builtin_amdgcn_readfirstlane(car + waves)) {
        typedef int v4i_t __attribute__((ext_vector_type(4)));
        v4i_t h;
        asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(h) : "s"(p.st.patch_pose + car) : "memory");
        const int a = h.z, b = h.w;
        if (h.x == RC_PATCH_SKIP) {              // reset observation is all zeros, dreamer/wrappers.py:413; a diverged car sees nothing
            v4u_t *out = reinterpret_cast<v4u_t *>(p.out.patch) + (size_t)car * 256u + lane;
            const v4u_t z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (NT) __builtin_nontemporal_store(z, out + 64 * g);
                else out[64 * g] = z;
            }
            continue;
        }
        // No tap can leave the image, and nothing is clamped, if the crop window lies inside the grid - or, with the zero border,
        // if the car's own cell does (the border is wider than any tap is far)
        const int lx = h.x - RCS_PATCH_WINDOW_I, ly = h.y - RCS_PATCH_WINDOW_I, span = 2 * RCS_PATCH_WINDOW_I - 1;
        const bool inside = pad ? ((unsigned)h.x < (unsigned)t.w && (unsigned)(h.y - 1) < (unsigned)t.h)
                                : (lx >= 0 && ly >= 0 && lx + span <= t.w - 1 && ly + span <= t.h - 1);
        const int icx = h.x + pad, icy = h.y + pad;            // the start cell in the image's coordinates
        // runs outside the corner blocks stay inside the window: |offset| <= (63 |a| + 31 |b|) / 2 + 1 on either axis (and with a, b exchanged)
        const int aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
        const int reach = (63 * (aa > ab ? aa : ab) + 31 * (aa > ab ? ab : aa)) / 2 + 2;
        const bool all_tested = reach > RCS_PATCH_WINDOW_I * 65536 - 2;
        if (inside) patch_car<false, NT>(p, img, car, lane, icx, icy, a, b, all_tested);
        else patch_car<true, NT>(p, img, car, lane, icx, icy, a, b, all_tested);
    }
}

// rc_patch_car_kernel's body for one workgroup of rc_patch_ts_kernel: p.trk's bitmap staged in LDS, then the cars list[first],
// list[first + stride], ... below `count` (first / stride count waves; the kernel above deals every car to the grid's waves in turn).
// A copy, not a shared function: the production kernel's code stays what it was.
template <bool NT>
__device__ __forceinline__ void patch_list_block(const RcParams &p, const int padded_bytes, const int32_t *list, const unsigned first,
                                                 const unsigned stride, const unsigned count) {
    extern __shared__ uint32_t lds_words[];
    const RcTrackDev &t = p.trk;
    const int pad = padded_bytes > 0 ? RC_PATCH_PAD : 0;
    PatchImage img;
    if (pad) {
        // the bitmap inside a border of `pad` zero cells (pad = 5 words: rows keep their word alignment)
        const int pw = (t.w + 2 * pad + 31) / 32, rows = t.h + 2 * pad;
        uint4 *d4 = reinterpret_cast<uint4 *>(lds_words);
        const uint4 z4 = {0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < (padded_bytes >> 4); i += blockDim.x) d4[i] = z4;
        __syncthreads();
        for (int i = threadIdx.x; i < t.h * t.pitch; i += blockDim.x) {
            const int row = i / t.pitch, word = i - row * t.pitch;
            if (word < pw - pad / 32) lds_words[(row + pad) * pw + pad / 32 + word] = t.drv_words[i];
        }
        img.pitch_b = (uint32_t)pw * 4u; img.w_cells = (uint32_t)(pw * 32); img.h_cells = (uint32_t)rows; img.zero_addr = 0u;
    } else {
        stage_bitmap(lds_words, t.drv_words, t.h * t.pitch + 1);        // + the all-zero word behind the bitmap (rc_load_track)
        img.pitch_b = (uint32_t)t.pitch * 4u; img.w_cells = (uint32_t)t.w; img.h_cells = (uint32_t)t.h;
        img.zero_addr = (uint32_t)(t.h * t.pitch) * 4u;
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    // cars are dealt to the waves of the grid in turn (a wave's cars are `waves` apart: neighbouring waves write
    // neighbouring patches).  The car is wave-uniform, so its header comes through the SCALAR unit: vector loads share one
    // in-order counter with the stores, and every car would start by waiting for the previous car's 4 KB to be
    // acknowledged.  (Inline assembly with its own wait: the compiler takes the load for a vector one because the kernel
    // also stores.)
    for (unsigned idx = __builtin_amdgcn_readfirstlane(first); idx < count; idx = __builtin_amdgcn_readfirstlane(idx + stride)) {
        unsigned car;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(car) : "s"(list + idx) : "memory");
        typedef int v4i_t __attribute__((ext_vector_type(4)));
        v4i_t h;
        asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(h) : "s"(p.st.patch_pose + car) : "memory");
        const int a = h.z, b = h.w;
        if (h.x == RC_PATCH_SKIP) {              // reset observation is all zeros, dreamer/wrappers.py:413; a diverged car sees nothing
            v4u_t *out = reinterpret_cast<v4u_t *>(p.out.patch) + (size_t)car * 256u + lane;
            const v4u_t z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (NT) __builtin_nontemporal_store(z, out + 64 * g);
                else out[64 * g] = z;
            }
            continue;
        }
        // No tap can leave the image, and nothing is clamped, if the crop window lies inside the grid - or, with the zero border,
        // if the car's own cell does (the border is wider than any tap is far)
        const int lx = h.x - RCS_PATCH_WINDOW_I, ly = h.y - RCS_PATCH_WINDOW_I, span = 2 * RCS_PATCH_WINDOW_I - 1;
        const bool inside = pad ? ((unsigned)h.x < (unsigned)t.w && (unsigned)(h.y - 1) < (unsigned)t.h)
                                : (lx >= 0 && ly >= 0 && lx + span <= t.w - 1 && ly + span <= t.h - 1);
        const int icx = h.x + pad, icy = h.y + pad;            // the start cell in the image's coordinates
        // runs outside the corner blocks stay inside the window: |offset| <= (63 |a| + 31 |b|) / 2 + 1 on either axis (and with a, b exchanged)
        const int aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
        const int reach = (63 * (aa > ab ? aa : ab) + 31 * (aa > ab ? ab : aa)) / 2 + 2;
        const bool all_tested = reach > RCS_PATCH_WINDOW_I * 65536 - 2;
        if (inside) patch_car<false, NT>(p, img, car, lane, icx, icy, a, b, all_tested);
        else patch_car<true, NT>(p, img, car, lane, icx, icy, a, b, all_tested);
    }
}


// The render with a track set: workgroups only render cars of the track whose bitmap they staged.  The grid of G workgroups is
// partitioned over the tracks in proportion to their car counts (ts_start, on the device): track k takes workgroups [F(k), F(k + 1)),
// F(k) = (tracks before k that have cars) + floor((G - T) start[k] / n), so that every track with cars has one at least (G >= T).
template <bool NT>
__global__ __launch_bounds__(1024) void rc_patch_ts_kernel(RcParams p0) {
    const int T = p0.ts_n, n = p0.n_cars, G = (int)gridDim.x, wg = (int)blockIdx.x;
    int k = -1, lo = 0, hi = 0, s0 = 0, s1 = 0, nonempty = 0;
#pragma unroll
    for (int j = 0; j < RC_TS_MAX; ++j) {
        if (j < T) {
            const int a = p0.ts_start[j], b = p0.ts_start[j + 1];
            const int f0 = nonempty + (int)((long long)(G - T) * a / n);
            nonempty += b > a ? 1 : 0;
            const int f1 = nonempty + (int)((long long)(G - T) * b / n);
            if (wg >= f0 && wg < f1) { k = j; lo = f0; hi = f1; s0 = a; s1 = b; }
        }
    }
    if (k < 0) return;
    const RcParams p = p0.ts_table[k];
    const unsigned per = blockDim.x >> 6;
    patch_list_block<NT>(p, p0.ts_pad_bytes[k], p0.ts_list + s0, (unsigned)(wg - lo) * per + (threadIdx.x >> 6), (unsigned)(hi - lo) * per,
                    (unsigned)(s1 - s0));
}

__global__ __launch_bounds__(256) void rc_set_pose_kernel(RcParams p, const float *__restrict__ xyyaw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_cars) return;
    const float x = xyyaw[3 * i], y = xyyaw[3 * i + 1], th = xyyaw[3 * i + 2];
    float sn, cs;
    sincos32(th, sn, cs);
    p.st.x[i] = x; p.st.y[i] = y; p.st.theta[i] = th; p.st.st[i] = sn; p.st.ct[i] = cs;
    p.st.scan_pose[i] = make_float4(x, y, cs, sn);
    if (p.render_patch) p.st.patch_pose[i] = patch_pose_of(p.trk, x, y, cs, sn, 0);
    p.st.fresh[i] = 0;
    p.out.fresh[i] = 0;
    float *pose = p.out.pose + 6 * i;
    pose[0] = x; pose[1] = y; pose[5] = th;
}

__global__ __launch_bounds__(256) void rc_random_actions_kernel(float *__restrict__ actions, int n_cars,
                                                                 uint32_t first_car, uint32_t seed_lo,
                                                                 uint32_t seed_hi, uint32_t step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cars) return;
    const rcd::u32x4 r = rcd::philox4x32(first_car + (uint32_t)i, step, 1u, 0u, seed_lo, seed_hi);
    const float u0 = (float)(r.x >> 8) * 5.9604644775390625e-8f;   // 2^-24
    const float u1 = (float)(r.y >> 8) * 5.9604644775390625e-8f;
    actions[2 * i] = u0 * 2.0f - 1.0f;
    actions[2 * i + 1] = u1 * 2.0f - 1.0f;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers
// Kernel timing without extra packets on the queue: the events handed to rck_set_launch_events are attached to the
// NEXT launch itself (hipExtLaunchKernelGGL: start / stop timestamps of the dispatch, what rocprofv3 reports), where a
// hipEventRecord before and after costs two barrier packets, ~3 us of device time per timed kernel.
// (the launch itself: `launch()` in racecar_internal.h, used by every unit)
namespace {
thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
}  // namespace

void rck_set_launch_events(hipEvent_t start, hipEvent_t stop) { g_ev_start = start; g_ev_stop = stop; }
void rck_take_launch_events(hipEvent_t *start, hipEvent_t *stop) { *start = g_ev_start; *stop = g_ev_stop; g_ev_start = g_ev_stop = nullptr; }

// ---- the order in which the scan takes the cars (RcStateDev::order): a counting sort by progress along the track, RC_ORDER_BUCKETS
// buckets; within a bucket the order is whatever the atomics give - results do not depend on it, every car is scanned on its own.
__device__ __forceinline__ int order_bucket(float progress) {
    // a key that is not a number (rows never written) or out of range lands in an end bucket: the order stays a permutation
    const float k = progress * (float)RC_ORDER_BUCKETS;
    if (!(k >= 0.0f)) return 0;
    return k >= (float)(RC_ORDER_BUCKETS - 1) ? RC_ORDER_BUCKETS - 1 : (int)k;
}
__global__ __launch_bounds__(256) void rc_order_count_kernel(const float *__restrict__ progress, int n, uint32_t *__restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&counts[order_bucket(progress[i])], 1u);
}
__global__ __launch_bounds__(RC_ORDER_BUCKETS) void rc_order_offsets_kernel(uint32_t *__restrict__ counts) {
    // exclusive prefix sum of the bucket counts, in place (one workgroup): the buckets' first positions
    __shared__ uint32_t s[RC_ORDER_BUCKETS];
    const int t = threadIdx.x;
    const uint32_t mine = counts[t];
    s[t] = mine;
    __syncthreads();
    for (int off = 1; off < RC_ORDER_BUCKETS; off <<= 1) {
        const uint32_t add = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    counts[t] = s[t] - mine;
}
__global__ __launch_bounds__(256) void rc_order_place_kernel(const float *__restrict__ progress, int n, uint32_t *__restrict__ cursor,
                                                             int32_t *__restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t pos = atomicAdd(&cursor[order_bucket(progress[i])], 1u);
    // Workgroups go to the 8 XCDs in turn.  Plain rank order would hand every XCD each eighth car of the stretch in flight - the same
    // table lines in all eight L2s; instead XCD x gets whole regions x, x + 8, ... of RC_ORDER_REGION ranks (region g, offset o ->
    // slot ((g / 8) R + o) 8 + g mod 8): the stretch in flight is the same, each L2 holds an eighth of it (1.8 % of the scan;
    // 64 and 512 ranks per region do 1.2 %, 1 024 and more lose - the XCDs' regions then differ too much in cost).
    pos = order_slot_of_rank(pos, (uint32_t)n);
    order[pos] = i;
}

// The key of the small batches' order: 1 - mean range / 15 m of the car's last scan, i.e. long rays (many trips) first - the
// waves that start last, when the first have freed their slots, are then the short ones (a wave per car).
__global__ __launch_bounds__(256) void rc_order_cost_key_kernel(const float *__restrict__ lidar, int n, float *__restrict__ key) {
    const int car = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (car >= n) return;
    float s = 0.0f;
    for (int b = lane; b < RC_N_BEAMS; b += 64) s += lidar[(size_t)car * RC_N_BEAMS + b];
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) key[car] = 1.0f - s * (0.999f / (15.0f * RC_N_BEAMS));
}
hipError_t rck_cost_keys(const float *lidar_dev, int n_cars, float *key_dev, hipStream_t s) {
    hipLaunchKernelGGL(rc_order_cost_key_kernel, dim3((unsigned)((n_cars + 3) / 4)), dim3(256), 0, s, lidar_dev, n_cars, key_dev);
    return hipGetLastError();
}

hipError_t rck_sort_cars(const float *progress_dev, int n_cars, uint32_t *counts_dev, int32_t *order_dev, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counts_dev, 0, sizeof(uint32_t) * RC_ORDER_BUCKETS, s);
    if (e != hipSuccess) return e;
    const int blocks = (n_cars + 255) / 256;
    hipLaunchKernelGGL(rc_order_count_kernel, dim3(blocks), dim3(256), 0, s, progress_dev, n_cars, counts_dev);
    hipLaunchKernelGGL(rc_order_offsets_kernel, dim3(1), dim3(RC_ORDER_BUCKETS), 0, s, counts_dev);
    hipLaunchKernelGGL(rc_order_place_kernel, dim3(blocks), dim3(256), 0, s, progress_dev, n_cars, counts_dev, order_dev);
    return hipGetLastError();
}

// ---- The lab library (racecar_lab.hip: scan variants 0-6, the stamps build): not part of this library.  It is looked for next
// to this one (libracecar_lab.so in the directory libracecar_hip.so was loaded from) the first time a handle asks for one of
// its kernels, and every such request fails with the reason when it is not there.
// What both sides of the lab boundary must agree on: the sizes of the structs that cross it by pointer and the hash of the
// headers that define them (-DRC_HEADERS_ID, build.py) - in ONE string, compared as a whole.
#ifndef RC_HEADERS_ID
#define RC_HEADERS_ID "unhashed"
#endif
const char *rck_lab_abi_string() {
    static const std::string s = "RcParams " + std::to_string(sizeof(RcParams)) + " RcLaunchInfo " + std::to_string(sizeof(RcLaunchInfo)) +
                                 " RcLabTables " + std::to_string(sizeof(RcLabTables)) + " headers " RC_HEADERS_ID;
    return s.c_str();
}

namespace {
struct Lab {
    void *handle = nullptr;
    int (*launch_raycast)(const RcParams *, const RcLaunchInfo *, const RcLabTables *, hipStream_t, hipEvent_t, hipEvent_t) = nullptr;
    int (*build_tables)(const RcTrackDev *, RcLabTables *) = nullptr;
    std::string why;                 // why it is not available
};
std::mutex g_lab_mutex;
Lab g_lab;

// A snapshot BY VALUE, taken under the lock (a reference to g_lab read after the lock was dropped raced with another
// thread inside lab() clearing `why` and assigning the function pointers).
Lab lab() {
    std::lock_guard<std::mutex> lock(g_lab_mutex);
    if (g_lab.handle != nullptr) return g_lab;
    g_lab.why.clear();               // (not loaded yet: look again - it may have been built since the last request)
    g_lab.launch_raycast = nullptr;
    g_lab.build_tables = nullptr;
    Dl_info info;
    std::string dir = ".";
    if (dladdr(reinterpret_cast<const void *>(&rck_set_launch_events), &info) != 0 && info.dli_fname != nullptr) {
        const std::string path(info.dli_fname);
        const size_t slash = path.rfind('/');
        if (slash != std::string::npos) dir = path.substr(0, slash);
    }
    const char *over = getenv("RC_LAB_LIBRARY");
    const std::string path = over != nullptr ? std::string(over) : dir + "/libracecar_lab.so";
    void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (h == nullptr) {
        const char *err = dlerror();              // (once: the call clears the message)
        g_lab.why = "the lab library is not built (" + path + ": " + std::string(err != nullptr ? err : "not found") +
                    "); build it with `python -m racing_dreamer_amd.build --lab`";
        return g_lab;
    }
    auto refuse = [&](const std::string &why) {
        g_lab.why = why;
        g_lab.launch_raycast = nullptr;
        g_lab.build_tables = nullptr;
        dlclose(h);
        return g_lab;
    };
    // RcParams, RcLaunchInfo and RcLabTables cross this boundary by pointer: a lab built against other headers reads them wrongly - wrong scans
    // or a GPU fault, no error.  The lab says what it was built against; anything else is refused.
    auto abi = reinterpret_cast<const char *(*)(void)>(dlsym(h, "rclab_abi"));
    const std::string want = rck_lab_abi_string();
    if (abi == nullptr || want != abi())
        return refuse(path + " was built against other headers (it says \"" + std::string(abi != nullptr ? abi() : "nothing: no rclab_abi") +
                      "\", this library needs \"" + want + "\"); rebuild it with `python -m racing_dreamer_amd.build --lab`");
    g_lab.launch_raycast = reinterpret_cast<decltype(g_lab.launch_raycast)>(dlsym(h, "rclab_launch_raycast"));
    g_lab.build_tables = reinterpret_cast<decltype(g_lab.build_tables)>(dlsym(h, "rclab_build_tables"));
    if (g_lab.launch_raycast == nullptr || g_lab.build_tables == nullptr)
        return refuse(path + " does not export rclab_launch_raycast / rclab_build_tables");
    g_lab.handle = h;
    return g_lab;
}
}  // namespace

// nullptr if the lab's kernels can be launched, else the reason (the calling thread's copy: valid until its next call)
const char *rck_lab_unavailable() {
    thread_local std::string reason;
    const Lab l = lab();
    if (l.handle != nullptr) return nullptr;
    reason = l.why;
    return reason.c_str();
}

// The tables of scan variants 1-5 for track `t`, built by the lab on the current device (rc_set_raycast_variant).
hipError_t rck_lab_build_tables(const RcTrackDev &t, RcLabTables *out) {
    const Lab l = lab();
    if (l.handle == nullptr) return hipErrorSharedObjectInitFailed;          // (rc_set_raycast_variant refuses before it comes to this)
    return (hipError_t)l.build_tables(&t, out);
}

// Run-time (cars per env, flag) -> template arguments: f gets a std::integral_constant / std::bool_constant and names the
// instantiation with its ::value.  Only what a launcher below spells is instantiated.
template <typename F>
inline void with_cars(int cars_per_env, F &&f) {
    switch (cars_per_env) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}
template <typename F>
inline void with_flag(bool on, F &&f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// The single-handle scan's instantiations, named in ONE place: what rck_launch_raycast launches, rck_scan_kernel_name spells and
// rck_set_lds_limits checks.  The bounded build (a validation band is in force: its trip loop counts its trips) never overlaps
// and has no noise (the ABI refuses the two together); LiDAR noise has instantiations of its own; else a small batch (several
// waves per car, few per SIMD) prepares the next round under the first request.
using ScanKernel = void (*)(RcParams, int);
struct ScanChoice { bool noise, guard, overlap; };
constexpr ScanChoice kScanChoices[] = {{false, false, false}, {false, false, true}, {false, true, false}, {true, false, false}, {true, false, true}};
static ScanChoice scan_choice(const RcParams &p, const RcLaunchInfo &li) { return {p.noise_on != 0, li.scan_guarded != 0, li.car_split > 1}; }
// The builds without overlap and without the bound have `split` = 1 and `part` = 0 compiled in (scan_one_wave_per_car,
// racecar_scan.h): a launch that hands such a build another split would scan 1 / split of the cars 'split' times over, silently.
// Every scan launcher asks this first.
static bool scan_split_fits(bool overlap, bool guard, int split) { return split >= 1 && (overlap || guard || split == 1); }
template <int A>
ScanKernel scan_kernel(const ScanChoice &c) {
    if (c.guard) return rc_raycast_car_kernel<A, false, true>;
    if (c.noise) return c.overlap ? rc_raycast_car_noise_kernel<A, true> : rc_raycast_car_noise_kernel<A, false>;
    return c.overlap ? rc_raycast_car_kernel<A, true, false> : rc_raycast_car_kernel<A, false, false>;
}
void rck_scan_kernel_name(const RcParams &p, const RcLaunchInfo &li, char *out, size_t bytes) {
    const ScanChoice c = scan_choice(p, li);
    const char *overlap = c.overlap ? "true" : "false";
    if (c.guard) snprintf(out, bytes, "rc_raycast_car_kernel<%d, false, true>", p.cars_per_env);
    else if (c.noise) snprintf(out, bytes, "rc_raycast_car_noise_kernel<%d, %s>", p.cars_per_env, overlap);
    else snprintf(out, bytes, "rc_raycast_car_kernel<%d, %s, false>", p.cars_per_env, overlap);
}

// The render and the scan address their dynamic LDS from LDS address 0: true only while they have no static LDS
static hipError_t no_static_lds(const void *k) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, k);
    return e == hipSuccess && fa.sharedSizeBytes != 0 ? hipErrorInvalidValue : e;
}
// ... and the render's bitmap needs more of it than a kernel gets unasked
static hipError_t raise_lds_ceiling(std::initializer_list<const void *> kernels, size_t lds_bytes) {
    for (const void *k : kernels) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e == hipSuccess) e = no_static_lds(k);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rck_set_lds_limits(size_t lds_bytes) {
    hipError_t e = raise_lds_ceiling({reinterpret_cast<const void *>(rc_patch_car_kernel<true>), reinterpret_cast<const void *>(rc_patch_car_kernel<false>)}, lds_bytes);
    for (int cars = 1; cars <= 4; ++cars)
        with_cars(cars, [&](auto a) {
            for (const ScanChoice &c : kScanChoices)
                if (e == hipSuccess) e = no_static_lds(reinterpret_cast<const void *>(scan_kernel<decltype(a)::value>(c)));
        });
    return e;
}

// The dynamics of one handle: by the env's track with a track set, with the vehicle parameters per car while vp_mode is on.
hipError_t rck_launch_dynamics(const RcParams &p, float *actions, int repeat, const RcRandomActions &ra, hipStream_t s) {
    const int threads = 256, blocks = (p.num_envs + threads - 1) / threads;
    const bool dr = p.vp_mode != RC_VP_OFF;
    with_cars(p.cars_per_env, [&](auto a) {
        constexpr int A = decltype(a)::value;
        auto go = [&](auto kernel) { launch(kernel, dim3(blocks), dim3(threads), 0, s, p, actions, repeat, ra.on, ra.seed_lo, ra.seed_hi, ra.step); };
        if (p.ts_n > 0) with_flag(dr, [&](auto d) { go(rc_dynamics_ts_kernel<A, decltype(d)::value>); });
        else if (dr) go(rc_dynamics_dr_kernel<A>);
        else go(rc_dynamics_kernel<A>);
    });
    return hipGetLastError();
}

hipError_t rck_launch_dynamics_group(const RcGroup &g, int cars_per_env, int repeat, const RcRandomActions &ra, hipStream_t s, bool dr) {
    const int waves = g.wave_start[g.n], blocks = (waves + 3) / 4;
    with_cars(cars_per_env, [&](auto a) {
        constexpr int A = decltype(a)::value;
        launch(dr ? rc_dynamics_dr_group_kernel<A> : rc_dynamics_group_kernel<A>, dim3(blocks), dim3(256), 0, s, g.params, g, repeat, ra.on, ra.seed_lo,
               ra.seed_hi, ra.step);
    });
    return hipGetLastError();
}

hipError_t rck_launch_raycast_group(const RcGroup &g, int cars_per_env, int split, hipStream_t s, bool noise) {
    const int waves = ((g.wave_start[g.n] + 7) / 8) * 8;     // one wave per workgroup, as the single-handle scan; whole turns of the 8 XCDs
    if (!scan_split_fits(split > 1, false, split)) return hipErrorInvalidValue;
    with_cars(cars_per_env, [&](auto a) {
        with_flag(split > 1, [&](auto o) {
            constexpr int A = decltype(a)::value;
            constexpr bool O = decltype(o)::value;
            launch(noise ? rc_raycast_group_noise_kernel<A, O> : rc_raycast_group_kernel<A, O>, dim3((unsigned)waves), dim3(64), (size_t)kCarLdsBytes, s,
                   g.params, g, split);
        });
    });
    return hipGetLastError();
}

// The reset of one handle: on the env's next track with a track set.
hipError_t rck_launch_reset(const RcParams &p, const uint8_t *mask_dev, hipStream_t s) {
    const int threads = 256, blocks = (p.num_envs + threads - 1) / threads;
    with_cars(p.cars_per_env, [&](auto a) {
        constexpr int A = decltype(a)::value;
        if (p.vp_mode == RC_VP_RANDOM)        // the new episode's vehicle parameters first: the draw reads the episode value the reset increments
            hipLaunchKernelGGL((rc_reset_dr_kernel<A>), dim3(blocks), dim3(threads), 0, s, p, mask_dev);
        launch(p.ts_n > 0 ? rc_reset_ts_kernel<A> : rc_reset_kernel<A>, dim3(blocks), dim3(threads), 0, s, p, mask_dev);
    });
    return hipGetLastError();
}

hipError_t rck_launch_raycast(const RcParams &p, const RcLaunchInfo &li, const RcLabTables *lab_tables, hipStream_t s) {
    const bool stamps = li.scan_stamps != nullptr && p.cars_per_env == 1;
    if (li.raycast_variant != 7 || stamps) {
        // a lab kernel (superseded variant or the instrumented build): racecar_lab.hip, loaded on first use
        const Lab l = lab();
        if (l.handle == nullptr) return hipErrorSharedObjectInitFailed;      // (rc_set_raycast_variant / rc_debug_scan_stamps refuse before it comes to this)
        hipEvent_t a, b;
        rck_take_launch_events(&a, &b);
        return (hipError_t)l.launch_raycast(&p, &li, lab_tables, s, a, b);
    }
    const ScanChoice choice = scan_choice(p, li);
    if (!scan_split_fits(choice.overlap, choice.guard, li.car_split)) return hipErrorInvalidValue;
    const int threads = li.car_threads, per = threads / 64;                     // waves per workgroup
    const long long waves = (long long)p.n_cars * li.car_split;
    with_cars(p.cars_per_env, [&](auto a) {
        launch(scan_kernel<decltype(a)::value>(scan_choice(p, li)), dim3((unsigned)((waves + per - 1) / per)), dim3(threads), (size_t)per * kCarLdsBytes, s, p, li.car_split);
    });
    return hipGetLastError();
}

// The render's workgroups: persistent, 16 waves each, the bitmap (lds_bytes) staged once per workgroup; as many as stay resident
static long long patch_blocks(const RcParams &p, const RcLaunchInfo &li, size_t lds_bytes) {
    const int per_cu = lds_bytes <= 80 * 1024 ? 2 : 1;
    const long long need = ((long long)p.n_cars + 15) / 16, resident = (long long)li.n_cu * per_cu;
    return need < resident ? need : resident;
}

hipError_t rck_launch_patch(const RcParams &p, const RcLaunchInfo &li, hipStream_t s) {
    const int padded = (li.patch_variant & 4) ? 0 : (int)rc_patch_padded_bytes(p.trk.h, p.trk.w);      // (4: experiment, the unpadded bitmap)
    const size_t lds = padded ? (size_t)padded : li.lds_bytes;
    const int blocks = (int)patch_blocks(p, li, lds);
    if (li.patch_variant & 2) launch(rc_patch_car_kernel<false>, dim3(blocks), dim3(1024), lds, s, p, padded);     // experiment: plain stores
    else launch(rc_patch_car_kernel<true>, dim3(blocks), dim3(1024), lds, s, p, padded);
    return hipGetLastError();
}

// ---- track set launchers (the dynamics and the reset: rck_launch_dynamics, rck_launch_reset)
hipError_t rck_launch_ts_list(const RcParams &p, hipStream_t s) {
    const dim3 blocks((unsigned)((p.n_cars + 255) / 256));
    hipLaunchKernelGGL(rc_ts_count_kernel, blocks, dim3(256), 0, s, p);
    hipLaunchKernelGGL(rc_ts_start_kernel, dim3(1), dim3(64), 0, s, p);
    hipLaunchKernelGGL(rc_ts_place_kernel, blocks, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t rck_launch_ts_raycast(const RcParams &p, const RcLaunchInfo &li, hipStream_t s) {
    const int split = li.car_split;
    const long long waves = (((long long)p.n_cars * split + 7) / 8) * 8;      // one wave per workgroup; whole turns of the 8 XCDs
    if (!scan_split_fits(split > 1, false, split)) return hipErrorInvalidValue;
    with_cars(p.cars_per_env, [&](auto a) {
        with_flag(split > 1, [&](auto o) {
            constexpr int A = decltype(a)::value;
            constexpr bool O = decltype(o)::value;
            launch(p.noise_on ? rc_raycast_ts_kernel<A, O, true> : rc_raycast_ts_kernel<A, O, false>, dim3((unsigned)waves), dim3(64), (size_t)kCarLdsBytes,
                   s, p, split);
        });
    });
    return hipGetLastError();
}

hipError_t rck_set_ts_lds_limit(size_t lds_bytes) {
    return raise_lds_ceiling({reinterpret_cast<const void *>(rc_patch_ts_kernel<true>), reinterpret_cast<const void *>(rc_patch_ts_kernel<false>)}, lds_bytes);
}

// lds_bytes: the largest bitmap image of the set's tracks (padded or not, per track); a workgroup at least for every track
hipError_t rck_launch_ts_patch(const RcParams &p, const RcLaunchInfo &li, size_t lds_bytes, hipStream_t s) {
    const long long resident = patch_blocks(p, li, lds_bytes), blocks = resident < p.ts_n ? p.ts_n : resident;
    if (li.patch_variant & 2) launch(rc_patch_ts_kernel<false>, dim3((unsigned)blocks), dim3(1024), lds_bytes, s, p);
    else launch(rc_patch_ts_kernel<true>, dim3((unsigned)blocks), dim3(1024), lds_bytes, s, p);
    return hipGetLastError();
}

hipError_t rck_launch_patch_exact(const RcExactParams &p0, int chunk_cars, hipStream_t s) {
    // a chunk of cars at a time: 387 KB of spline coefficients per car in flight (two kernels per chunk: the prefilter, then the
    // rotation + resize); the launch timer spans the first launch's start to the last one's end
    hipEvent_t a, b;
    rck_take_launch_events(&a, &b);
    RcExactParams p = p0;
    for (int c0 = 0; c0 < p0.n_cars; c0 += chunk_cars) {
        const int n = p0.n_cars - c0 < chunk_cars ? p0.n_cars - c0 : chunk_cars;
        p.car0 = c0;
        hipExtLaunchKernelGGL(rc_patch_exact_prefilter_kernel, dim3(n), dim3(256), 0u, s, c0 == 0 ? a : nullptr, nullptr, 0u, p);
        if (p.check) hipExtLaunchKernelGGL(rc_patch_exact_sample_kernel<true>, dim3(n), dim3(PX_ST), 0u, s, nullptr, c0 + n >= p0.n_cars ? b : nullptr, 0u, p);
        else hipExtLaunchKernelGGL(rc_patch_exact_sample_kernel<false>, dim3(n), dim3(PX_ST), 0u, s, nullptr, c0 + n >= p0.n_cars ? b : nullptr, 0u, p);
    }
    return hipGetLastError();
}

hipError_t rck_launch_set_pose(const RcParams &p, const float *xyyaw_dev, hipStream_t s) {
    const int threads = 256, blocks = (p.n_cars + threads - 1) / threads;
    launch(rc_set_pose_kernel, dim3(blocks), dim3(threads), 0, s, p, xyyaw_dev);
    return hipGetLastError();
}

hipError_t rck_launch_selftest_div6(int blocks, int threads, int per_lane, unsigned long long *mismatches_dev, hipStream_t s) {
    hipLaunchKernelGGL(rc_selftest_div6_kernel, dim3(blocks), dim3(threads), 0, s, 0x243f6a8885a308d3ull, per_lane, mismatches_dev);
    return hipGetLastError();
}

hipError_t rck_launch_selftest_rcp(uint32_t exp_lo, uint32_t exp_hi, unsigned long long *mismatches_dev, hipStream_t s) {
    hipLaunchKernelGGL(rc_selftest_rcp_kernel, dim3(4096), dim3(256), 0, s, exp_lo, exp_hi, mismatches_dev);
    return hipGetLastError();
}

hipError_t rck_launch_random_actions(float *actions, int n_cars, uint32_t first_car, uint32_t seed_lo,
                                     uint32_t seed_hi, uint32_t step, hipStream_t s) {
    const int threads = 256, blocks = (n_cars + threads - 1) / threads;
    launch(rc_random_actions_kernel, dim3(blocks), dim3(threads), 0, s, actions, n_cars, first_car, seed_lo, seed_hi, step);
    return hipGetLastError();
}