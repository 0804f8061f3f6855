// rc_look_ahead: what would really happen from here under these actions?  K candidate action sequences of H agent steps per
// env, every one carried through the env's true dynamics from its live state, in one launch and without touching that state
// (include/racecar_hip.h).
//
//   rc_look_ahead_kernel<A, DR, TS, NS>  one lane per (env, candidate): the env's cars, its step counters and - NS - its
//                       n_step_progress windows are copied once, into registers and LDS, and stepped H times by the sub-step
//                       the dynamics kernel runs (dynamics_substep, racecar_step.h: one body, two instantiations).  The
//                       actions are given, so no scan is needed; a finished env is frozen (reward +0.0f, flags kept), never
//                       reset.  Reads the simulator's state, its vehicle parameters and track ids; writes only the caller's
//                       output arrays.
//
// DR: the vehicle parameters per car (rc_set_vehicle_randomization / rc_set_vehicle_params), TS: the env's current track of a
// track set - as the dynamics kernel's.  NS: some car slot runs n_step_progress: its window is indexed by steps % n_steps, a
// lane value, so the private copy lives in LDS, [slot][k][lane] (a lane's column: no bank conflict whatever k the lanes hold).
#include "racecar_step.h"

#define RC_LA_THREADS 128                       // lanes per workgroup: the windows of 4 slots take 4 x 16 x 128 x 4 = 32 KB of LDS

namespace {

__device__ __forceinline__ uint32_t la_flags(const Car &c) {
    return (uint32_t)(c.done != 0) | (uint32_t)(c.trunc != 0) << 1 | (uint32_t)(c.wall != 0) << 2 | (uint32_t)(c.opp != 0) << 3 |
           (uint32_t)(c.wrong != 0) << 4;
}

template <int A, bool DR, bool TS, bool NS>
__global__ __launch_bounds__(RC_LA_THREADS) void rc_look_ahead_kernel(RcParams p, RcLookAhead c) {
    __shared__ float win[NS ? A * RC_NSTEP_MAX * RC_LA_THREADS : 1];
    const int lane = blockIdx.x * RC_LA_THREADS + threadIdx.x;       // (E K fits int32: rc_look_ahead refuses more)
    if (lane >= c.lanes) return;
    const int e = lane / c.candidates;
    RcTrackDev t_l = {};
    if (TS) lane_track(p, ts_track_of(p, e), t_l);
    const RcTrackDev &t = TS ? t_l : p.trk;
    Car car[A];
    load_cars<A>(p, e, car);
    int steps = p.st.steps[e], agent_steps = p.st.agent_steps[e];
    float vp[A][RC_VP_COUNT];
    if (DR) {
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int i = 0; i < RC_VP_COUNT; ++i) vp[a][i] = p.vparams[(size_t)(e * A + a) * RC_VP_COUNT + i];
    }
    if (NS) {
#pragma unroll
        for (int a = 0; a < A; ++a)
            if (p.car_task[a] == 2) {
                const float *h = p.st.nstep_hist + (size_t)(e * A + a) * RC_NSTEP_MAX;
#pragma unroll
                for (int k = 0; k < RC_NSTEP_MAX; ++k) win[(a * RC_NSTEP_MAX + k) * RC_LA_THREADS + threadIdx.x] = h[k];
            }
    }
    bool fin = false;
#pragma unroll
    for (int a = 0; a < A; ++a) fin |= car[a].done != 0;
    const int H = c.horizon;
    const size_t row0 = (size_t)lane * H * A;                      // the lane's first (step, slot) row of the [E, K, H, A, .] arrays
    float ret[A];
#pragma unroll
    for (int a = 0; a < A; ++a) ret[a] = 0.0f;
    int length = 0;
    for (int ts = 0; ts < H; ++ts) {
        const size_t row = row0 + (size_t)ts * A;
#pragma unroll
        for (int a = 0; a < A; ++a) car[a].rew = 0.0f;
        if (!fin) {
            float motor[A], steer[A];
#pragma unroll
            for (int a = 0; a < A; ++a) controls_of(p, c.actions[2 * (row + a)], c.actions[2 * (row + a) + 1], motor[a], steer[a]);
            for (int sub = 0; sub < c.repeat; ++sub) {   // ActionRepeat, as dynamics_env
                const bool stop = dynamics_substep<A, DR>(p, t, car, motor, steer, vp, steps, [&](int a, int k) -> float & {
                    return win[NS ? (a * RC_NSTEP_MAX + k) * RC_LA_THREADS + threadIdx.x : 0];
                });
                if (stop) break;
            }
            agent_steps += 1;
            if (p.time_limit_steps > 0 && agent_steps >= p.time_limit_steps) {   // TimeLimit, as dynamics_env
#pragma unroll
                for (int a = 0; a < A; ++a) { car[a].done = 1; car[a].trunc = 1; }
            }
#pragma unroll
            for (int a = 0; a < A; ++a) fin |= car[a].done != 0;
            length = ts + 1;
        }
#pragma unroll
        for (int a = 0; a < A; ++a) {
            ret[a] = ret[a] + car[a].rew;
            if (c.reward) c.reward[row + a] = car[a].rew;
            if (c.flags) c.flags[row + a] = (uint8_t)la_flags(car[a]);
            if (c.pose) {
                float *q = c.pose + 3 * (row + a);
                q[0] = car[a].x; q[1] = car[a].y; q[2] = car[a].th;
            }
        }
    }
    if (c.length) c.length[lane] = length;
    const float time = (float)steps * RCS_DT;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const size_t i = (size_t)lane * A + a;
        if (c.ret) c.ret[i] = ret[a];
        if (c.final_state) {
            float *q = c.final_state + 8 * i;
            q[0] = car[a].x; q[1] = car[a].y; q[2] = car[a].th; q[3] = car[a].v; q[4] = car[a].dl; q[5] = car[a].om;
            q[6] = (float)(car[a].lap - 1) + car[a].pr; q[7] = time;
        }
    }
}

template <int A, bool DR, bool TS>
void la_launch(const RcParams &p, const RcLookAhead &c, bool ns, hipStream_t s) {
    const dim3 grid((unsigned)((c.lanes + RC_LA_THREADS - 1) / RC_LA_THREADS)), block(RC_LA_THREADS);
    if (ns) launch(rc_look_ahead_kernel<A, DR, TS, true>, grid, block, 0, s, p, c);
    else launch(rc_look_ahead_kernel<A, DR, TS, false>, grid, block, 0, s, p, c);
}

template <int A>
void la_launch_cars(const RcParams &p, const RcLookAhead &c, bool ns, hipStream_t s) {
    const bool dr = p.vp_mode != RC_VP_OFF, ts = p.ts_n > 0;
    if (ts) { if (dr) la_launch<A, true, true>(p, c, ns, s); else la_launch<A, false, true>(p, c, ns, s); }
    else { if (dr) la_launch<A, true, false>(p, c, ns, s); else la_launch<A, false, false>(p, c, ns, s); }
}

}  // namespace

hipError_t rck_launch_look_ahead(const RcParams &p, const RcLookAhead &c, hipStream_t s) {
    bool ns = false;
    for (int a = 0; a < p.cars_per_env; ++a) ns |= p.car_task[a] == 2;
    switch (p.cars_per_env) {
        case 1: la_launch_cars<1>(p, c, ns, s); break;
        case 2: la_launch_cars<2>(p, c, ns, s); break;
        case 3: la_launch_cars<3>(p, c, ns, s); break;
        case 4: la_launch_cars<4>(p, c, ns, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
