// One sub-step of the env's dynamics and what surrounds it that does not depend on who steps: the load of an env's cars, the
// env's track in a track set, the action convention.  A header, because two units instantiate it: racecar_kernels.hip - the
// step's dynamics kernel, which carries the live env one agent step on - and racecar_lookahead.hip, which carries private
// copies of it through a whole horizon (rc_look_ahead).  The operations and their order are the spec's: whoever
// steps computes the same bits.
#pragma once
#include "racecar_car.h"

namespace {

template <int A>
__device__ __forceinline__ void load_cars(const RcParams &p, int e, Car (&car)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const int i = e * A + a;
        Car &c = car[a];
        c.x = p.st.x[i]; c.y = p.st.y[i]; c.th = p.st.theta[i]; c.ct = p.st.ct[i]; c.st = p.st.st[i];
        c.v = p.st.v[i]; c.dl = p.st.delta[i]; c.om = p.st.omega[i]; c.ac = p.st.accel[i];
        c.pr = p.st.progress[i]; c.lap = p.st.lap[i]; c.cp = p.st.cp[i];
        c.wall = p.st.wall[i]; c.opp = p.st.opp[i]; c.wrong = p.st.wrong[i];
        c.done = p.st.done[i]; c.trunc = p.st.trunc[i]; c.fresh = 0;
        c.rew = 0.0f;
    }
}

// ---- track set (rc_set_track_set): the env's track k is a lane value; the dynamics reads the few fields of track k's RcTrackDev
// that it uses (walls, progress grid, spawn table, geometry) with per-lane loads from the owner's table, the rest stays zero.
__device__ __forceinline__ int ts_track_of(const RcParams &p, int e) {
    const int k = p.ts_track[e];
    return (unsigned)k < (unsigned)p.ts_n ? k : 0;          // (a value written from outside [0, T) reads as track 0)
}

__device__ __forceinline__ void lane_track(const RcParams &p, int k, RcTrackDev &t) {
    const RcTrackDev &s = p.ts_table[k].trk;
    t.ray_words = s.ray_words; t.progress = s.progress; t.spawn = s.spawn;
    t.w = s.w; t.h = s.h; t.pitch = s.pitch; t.n_centerline = s.n_centerline;
    t.org_x = s.org_x; t.org_y = s.org_y; t.inv_res = s.inv_res;
}

// The action convention: what the integrator takes for the pair (a0, a1) the caller gave.
__device__ __forceinline__ void controls_of(const RcParams &p, float a0, float a1, float &motor, float &steer) {
    float m = a0, s = a1;
    if (p.remap_actions) {   // ReduceActionSpace, dreamer/wrappers.py:128-130
        m = ((a0 + 1.0f) * 0.5f) * (p.act_hi0 - p.act_lo0) + p.act_lo0;
        s = ((a1 + 1.0f) * 0.5f) * (p.act_hi1 - p.act_lo1) + p.act_lo1;
    }
    motor = clampf(m, -1.0f, 1.0f);
    steer = clampf(s, -1.0f, 1.0f);
}

// One sub-step of the cars of one env on track t (the body: racecar_substep.inc, which dynamics_env includes as text): adds the sub-step's
// reward to Car::rew, counts `steps`, returns whether the env finished on this sub-step (the caller's action repeat breaks
// there).  DR: the five vehicle parameters of the integrator come from vp instead of the spec's constants - the same operations
// in the same order, only the operand differs.  hist(a, k): slot k of car slot a's n_step_progress window (read and written
// only where car_task[a] is that task) - the live env's window in global memory for the step, a private copy for a look-ahead.
template <int A, bool DR, typename Hist>
__device__ __forceinline__ bool dynamics_substep(const RcParams &p, const RcTrackDev &t, Car (&car)[A], const float (&motor)[A],
                                                 const float (&steer)[A], const float (&vp)[A][RC_VP_COUNT], int &steps, Hist &&hist) {
#define RC_NSTEP_SLOT(a, k) (&hist(a, k))
#include "racecar_substep.inc"
#undef RC_NSTEP_SLOT
    return stop;
}

}  // namespace
