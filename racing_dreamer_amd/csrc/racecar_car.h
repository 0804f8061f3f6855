// The car of the step's dynamics and what both the step and the spawn-table builder ask of it: its cell, the progress value
// there, the footprint test against the walls and the car-car overlap (racecar_kernels.hip, racecar_tracks.hip).
#pragma once
#include "racecar_scan.h"

namespace {

__device__ __forceinline__ void cell_of(const RcTrackDev &t, float wx, float wy, int &ix, int &iy) {
    ix = (int)floorf((wx - t.org_x) * t.inv_res);
    iy = (int)floorf((wy - t.org_y) * t.inv_res);
}

__device__ __forceinline__ float progress_at(const RcTrackDev &t, float wx, float wy) {
    int ix, iy;
    cell_of(t, wx, wy, ix, iy);
    // branch-free (an off-grid car reads cell (0, 0) and discards it), so the load is issued next to the footprint's
    const bool inb = (unsigned)ix < (unsigned)t.w && (unsigned)iy < (unsigned)t.h;
    const float pr = t.progress[inb ? iy * t.w + ix : 0];
    return inb ? pr : -1.0f;
}

struct Car {
    float x, y, th, ct, st, v, dl, om, ac, pr, rew;
    int lap, cp;
    int wall, opp, wrong, done, trunc, fresh;
};

// Footprint perimeter vs occupancy (H5): the 34 border points of the 12 x 7 body lattice (0.05 m pitch, rear axle at
// lattice node (2, 3)) in 16.16 fixed-point cell coordinates - oracle/racecar_oracle.py, _wall_hit.  With the lattice
// vectors e = rne(65536 k (cos, sin)) and f = (-e.y, e.x) a point is two integer multiply-adds of the rear-axle
// position, its cell two shifts, and "outside the grid counts as wall" is one unsigned min per axis: a negative or
// too large index clamps to the last row / column, which belongs to the sentinel ring and is always set.  About 10
// vector instructions per point, all 34 words requested back to back and waited for once (the fp32 rotation +
// floor + bounds select of the first version took 30 per point: 2/3 of the kernel, which runs one wave per SIMD and
// is therefore bound by its own instruction stream).
__device__ __forceinline__ int wall_hit(const RcTrackDev &t, const Car &c) {
    const float k = RCS_FOOT_STEP * t.inv_res;
    const float gx = (c.x - t.org_x) * t.inv_res, gy = (c.y - t.org_y) * t.inv_res;
    const bool bad = !(fabsf(gx) <= 8192.0f && fabsf(gy) <= 8192.0f);      // not a position: counts as contact
    const int ex = (int)__builtin_rintf((c.ct * k) * 65536.0f), ey = (int)__builtin_rintf((c.st * k) * 65536.0f);
    const int x0 = (int)__builtin_rintf(gx * 65536.0f), y0 = (int)__builtin_rintf(gy * 65536.0f);
    const uint32_t wm1 = (uint32_t)(t.w - 1), hm1 = (uint32_t)(t.h - 1);
    uint32_t hit = bad ? 1u : 0u;
    auto probe = [&](int li, int lj) {
        const int px = x0 + (li - 2) * ex - (lj - 3) * ey, py = y0 + (li - 2) * ey + (lj - 3) * ex;
        const uint32_t ix = min((uint32_t)(px >> 16), wm1), iy = min((uint32_t)(py >> 16), hm1);
        hit |= t.ray_words[iy * (uint32_t)t.pitch + (ix >> 5)] >> (ix & 31u);
    };
#pragma unroll
    for (int i = 0; i < 12; ++i) { probe(i, 0); probe(i, 6); }
#pragma unroll
    for (int j = 1; j < 6; ++j) { probe(0, j); probe(11, j); }
    return (int)(hit & 1u);
}

// Oriented-rectangle overlap by separating axes (car-car collision, H5/H18).
__device__ __forceinline__ int obb_overlap(const Car &a, const Car &b) {
    const float ax = a.x + RCS_BOX_CX * a.ct, ay = a.y + RCS_BOX_CX * a.st;
    const float bx = b.x + RCS_BOX_CX * b.ct, by = b.y + RCS_BOX_CX * b.st;
    const float dx = bx - ax, dy = by - ay;
    const float c = fabsf(a.ct * b.ct + a.st * b.st);
    const float s = fabsf(a.st * b.ct - a.ct * b.st);
    const float ra = RCS_BOX_HL + (RCS_BOX_HL * c + RCS_BOX_HW * s);
    const float rb = RCS_BOX_HW + (RCS_BOX_HL * s + RCS_BOX_HW * c);
    bool sep = fabsf(dx * a.ct + dy * a.st) > ra;
    sep |= fabsf(dy * a.ct - dx * a.st) > rb;
    sep |= fabsf(dx * b.ct + dy * b.st) > ra;
    sep |= fabsf(dy * b.ct - dx * b.st) > rb;
    return sep ? 0 : 1;
}

}  // namespace
