// A track's device tables, built and checked at rc_load_track: the spawn table, the scan's first-trip table and quadrant
// planes, and the validation of the latter two by a bounded scan from every free cell.
#include <cmath>

#include "racecar_car.h"

namespace {

// The spawn table (RcTrackDev::spawn): per row the pose, sin / cos of its heading (the spec's sincos32), the progress value of
// its cell, its checkpoint (+ the anchor bin of a multi-car start, see below), and the room a random start has there - computed
// once per track ON THE DEVICE with the very functions a reset would call, so the centre-line part of a reset is one 32-byte
// gather with no arithmetic behind it.
//   Row i is centre-line bin u(i) = the first USABLE bin among i, i + 1, ... (around the lap, RCS_SPAWN_SAFE_SEARCH of them; i if
// none): usable = the footprint test of H5 on the bin's own pose finds no wall (oracle: spawn_usable, spawn_rows).  On hand-drawn
// maps with boxes on the track the most central cell of a BFS distance bin can lie where a car does not fit; no start goes there.
//   Lateral room (oracle: spawn_width): d2 = squared cell distance from the point's cell to the nearest cell that is not drivable
// (outside the grid included) in the window of +- RCS_SPAWN_CLEAR_R cells, at most (R + 1)^2;
// w = clamp(isqrt(d2) * res - RCS_SPAWN_MARGIN, 0, RCS_SPAWN_W_MAX) - integers up to the last two operations.
//   Heading room (oracle: spawn_heading_room): RCS_HEADING_JITTER where w > 0 (the margin holds for every heading); where w = 0,
// HEADING_ROOM[k], k = the smallest over the 34 footprint points of isqrt(squared cell distance to the nearest non-drivable cell
// within +- RCS_SPAWN_FOOT_R), capped at 5.  The row's last word holds w if w > 0, else - (heading room): one float, no bit fields.
__device__ __forceinline__ void foot_cell(const RcTrackDev &t, float x, float y, float ct, float st, int li, int lj, int &ix, int &iy) {
    const float k = RCS_FOOT_STEP * t.inv_res;
    const float gx = (x - t.org_x) * t.inv_res, gy = (y - t.org_y) * t.inv_res;
    const int ex = (int)__builtin_rintf((ct * k) * 65536.0f), ey = (int)__builtin_rintf((st * k) * 65536.0f);
    const int x0 = (int)__builtin_rintf(gx * 65536.0f), y0 = (int)__builtin_rintf(gy * 65536.0f);
    ix = (x0 + (li - 2) * ex - (lj - 3) * ey) >> 16;
    iy = (y0 + (li - 2) * ey + (lj - 3) * ex) >> 16;
}

template <typename F>
__device__ __forceinline__ void for_each_foot_point(F &&f) {
    for (int i = 0; i < 12; ++i) { f(i, 0); f(i, 6); }
    for (int j = 1; j < 6; ++j) { f(0, j); f(11, j); }
}

__device__ __noinline__ bool bin_usable(const RcTrackDev &t, int i) {
    Car c;
    c.x = t.centerline[4 * i]; c.y = t.centerline[4 * i + 1];
    sincos32(t.centerline[4 * i + 2], c.st, c.ct);
    return wall_hit(t, c) == 0;
}

__global__ __launch_bounds__(256) void rc_build_spawn_kernel(RcTrackDev t, float4 *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t.n_centerline;
    if (i >= n) return;
    int u = i;
    for (int s = 0; s < RCS_SPAWN_SAFE_SEARCH && s < n; ++s)
        if (bin_usable(t, (i + s) % n)) { u = (i + s) % n; break; }
    const float x = t.centerline[4 * u], y = t.centerline[4 * u + 1], th = t.centerline[4 * u + 2];
    float sn, cs;
    sincos32(th, sn, cs);
    float pr = progress_at(t, x, y);
    pr = pr < 0.0f ? 0.0f : pr;
    int cp = (int)(pr * (float)RCS_N_CHECKPOINTS);
    cp = cp < RCS_N_CHECKPOINTS - 1 ? cp : RCS_N_CHECKPOINTS - 1;
    auto clearance2 = [&](int ix, int iy, int R) {           // squared cell distance to the nearest non-drivable cell within +- R
        int d2 = (R + 1) * (R + 1);
        if (!((unsigned)ix < (unsigned)t.w && (unsigned)iy < (unsigned)t.h)) return 0;
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                const int jx = ix + dx, jy = iy + dy;
                const bool inside = (unsigned)jx < (unsigned)t.w && (unsigned)jy < (unsigned)t.h;
                const bool blocked = !inside || bit_at(t.drv_words, t.pitch, jx, jy) == 0;
                const int q = dx * dx + dy * dy;
                d2 = (blocked && q < d2) ? q : d2;
            }
        return d2;
    };
    auto isqrt = [](int d2) { int k = 0; while ((k + 1) * (k + 1) <= d2) ++k; return k; };
    int ix, iy;
    cell_of(t, x, y, ix, iy);
    const float w = clampf((float)isqrt(clearance2(ix, iy, RCS_SPAWN_CLEAR_R)) * t.res - RCS_SPAWN_MARGIN, 0.0f, RCS_SPAWN_W_MAX);
    float room = w;
    if (!(w > 0.0f)) {
        int kmin = RCS_SPAWN_FOOT_R;
        for_each_foot_point([&](int li, int lj) {
            int px, py;
            foot_cell(t, x, y, cs, sn, li, lj, px, py);
            const int k = isqrt(clearance2(px, py, RCS_SPAWN_FOOT_R));
            kmin = k < kmin ? k : kmin;
        });
        const float rooms[6] = RCS_HEADING_ROOM_INIT;
        room = -rooms[kmin];
    }
    // Where a multi-car start drawn at this bin really goes (oracle: spawn_safe): the first bin j among i, i + 1, ... (around the
    // lap, RCS_SPAWN_SAFE_SEARCH of them) at which the centre-line poses of RC_MAX_CARS cars RCS_BALL_GAP_BINS apart touch no wall
    // and do not overlap pairwise; i itself if there is none.  Where the progress grid's wavefronts fold (columbia_slam's last bins
    // run back along the bins before them) bins 1.2 m apart along the table are centimetres apart on the ground.
    int safe = i;
    for (int s = 0; s < RCS_SPAWN_SAFE_SEARCH && s < n; ++s) {
        const int j = (i + s) % n;
        Car c[4];
        int clash = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int idx = (j - a * RCS_BALL_GAP_BINS) % n;
            if (idx < 0) idx += n;
            c[a].x = t.centerline[4 * idx]; c[a].y = t.centerline[4 * idx + 1];
            sincos32(t.centerline[4 * idx + 2], c[a].st, c[a].ct);
            clash |= bin_usable(t, idx) ? 0 : 1;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b) clash |= obb_overlap(c[a], c[b]);
        if (!clash) { safe = j; break; }
    }
    out[2 * i] = make_float4(x, y, th, cs);
    out[2 * i + 1] = make_float4(sn, pr, __int_as_float(cp | (safe << 8)), room);      // checkpoint < 256; the bin above it
}

// ---- First-trip table (RcTrackDev::first_rect) --------------------------------------------------------------
// All 1080 rays of a car start in the same cell, so the FIRST rectangle of every ray can come from a much richer
// table than the four quadrant planes without any cache cost: a car reads one 512-byte line per step.  Per cell
// the line holds RC_FIRST_PLANES = 4 quadrants x RC_FIRST_BINS entries, the bin being the ray's slope |dy / dx|
// in eight steps per octave over 2^-4 .. 2^4 (the outer bins open-ended): exactly what the scan gets from the float
// bits of |dy| * |1 / dx| (exponent and three mantissa bits) in two instructions.  An entry is a rectangle anchored at the cell like the plane entries, but
// it only has to be free INSIDE THE SECTOR that rays of its bin can touch (start point anywhere in the cell, slope
// anywhere in the bin, both widened by a margin far above the traversal's rounding) - its far corners may lie
// inside walls.  The exit arithmetic is unchanged: a ray of that bin visits only sector cells before it leaves
// the rectangle, and those are free.  A ray heading down a diagonal straight thus crosses it in one trip where
// fully free rectangles need one per stair of the wall.  tools/analysis/skip_stats.py firsttrip-slope / sector: 3.1 trips for the slowest
// ray of a wave on austria against 4.1 with the quadrant planes alone; specialising the later trips as well
// would need the big table in L2 and gain little more (tools/analysis/skip_stats.py firsttrip-angle).
//
// Bin parameters (set by rck_build_first_table): slope range in the bin's own frame (bins >= RC_FIRST_BINS / 2 are
// y-dominant and handled with the axes swapped, slope = |dx / dy|) and 1/cos, 1/sin of two sample directions.
struct RcFirstBin { float s1, s2, ka0, kb0, ka1, kb1; };
__constant__ RcFirstBin c_first_bins[RC_FIRST_BINS];

// One thread per (cell, quadrant, bin).  Column c of the rectangle (offset along the bin's dominant axis) is touched
// by rays of the bin in rows floor(s1 (c - 1) - 0.01) .. floor(1 + s2 (c + 1) + 0.01): the ray is inside column c
// for travelled distances in (c - 1, c + 1) along the dominant axis and starts anywhere in [0, 1]^2.  The first
// stop cell in that range caps the height of every rectangle that includes the column; among the rectangles
// (c + 1) x cap(c) the one at whose exit the most sample rays stop is kept, then the one with the largest summed exit
// distance for two sample directions.
__global__ __launch_bounds__(256) void rc_build_first_kernel(RcTrackDev t, uint16_t *__restrict__ out) {
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned total = (unsigned)t.h * (unsigned)t.w * RC_FIRST_PLANES;
    if (gid >= total) return;
    const int bin = (int)(gid % RC_FIRST_BINS), q = (int)((gid / RC_FIRST_BINS) & 3u);
    const unsigned cell = gid / RC_FIRST_PLANES;
    const int ix = (int)(cell % (unsigned)t.w), iy = (int)(cell / (unsigned)t.w);
    uint16_t &e = out[((size_t)iy * t.cell_pitch + ix) * RC_FIRST_PLANES + q * RC_FIRST_BINS + bin];
    if (ix == 0 || iy == 0 || ix == t.w - 1 || iy == t.h - 1) { e = 0x0100; return; }     // sentinel ring: "no return"
    if (bit_at(t.ray_words, t.pitch, ix, iy)) { e = 0; return; }                            // wall
    const int sx = (q & 1) ? -1 : 1, sy = (q & 2) ? -1 : 1;       // plane group q = (dy < 0) * 2 + (dx < 0)
    const bool swap = bin >= RC_FIRST_BINS / 2;
    const RcFirstBin b = c_first_bins[bin];
    const int cap = 255;
    int hmax = cap, bw = 1, bh = 1;
    float best = -1.0f;
    for (int c = 0; c < cap; ++c) {
        const int lo = max(0, (int)floorf(b.s1 * (float)max(0, c - 1) - 0.01f));
        const int hi = min(hmax - 1, (int)floorf(1.0f + b.s2 * (float)(c + 1) + 0.01f));
        for (int r = lo; r <= hi; ++r) {
            const int x = swap ? ix + sx * r : ix + sx * c, y = swap ? iy + sy * c : iy + sy * r;
            const bool stop = (unsigned)x >= (unsigned)t.w || (unsigned)y >= (unsigned)t.h || bit_at(t.ray_words, t.pitch, x, y);
            if (stop) { hmax = r; break; }
        }
        if (hmax <= 0) break;
        const int pw = swap ? hmax : c + 1, ph = swap ? c + 1 : hmax;          // extents along x and y
        float sc = fminf((float)pw * b.ka0, (float)ph * b.kb0) + fminf((float)pw * b.ka1, (float)ph * b.kb1);
        // ... after the number of sample rays (from the cell centre, five slopes across the bin) that STOP where they leave
        // the rectangle, i.e. whose exit cell is a stop cell: such a ray is finished after one trip, and a wave's round is as
        // long as its slowest ray (A/B on one box: 0.1845 -> 0.181 ms; the longest rectangle is not the one with the fewest
        // second trips - thinner sectors from sub-cell start positions made longer rectangles AND more trips)
        int stops = 0;
        for (int k = 0; k < 5; ++k) {
            const float m = b.s1 + (b.s2 - b.s1) * (0.1f + 0.2f * (float)k);         // own-frame slope (rows per column)
            const float yfar = 0.5f + m * ((float)c + 0.5f);
            int ec, er;                                                                 // exit cell, own-frame (column, row)
            if (yfar < (float)hmax) { ec = c + 1; er = (int)floorf(yfar); }
            else { ec = (int)floorf(0.5f + ((float)hmax - 0.5f) / fmaxf(m, 1e-6f)); er = hmax; }
            const int x = swap ? ix + sx * er : ix + sx * ec, y = swap ? iy + sy * ec : iy + sy * er;
            stops += ((unsigned)x >= (unsigned)t.w || (unsigned)y >= (unsigned)t.h || bit_at(t.ray_words, t.pitch, x, y)) ? 1 : 0;
        }
        sc += 1.0e4f * (float)stops;
        if (sc > best) { best = sc; bw = pw; bh = ph; }
    }
    e = (uint16_t)(bw | (bh << 8));
}

// ---- Quadrant planes (RcTrackDev::quad_rect), built on the device --------------------------------------------------
// Free run length from every cell towards -x and towards +x (capped at 255; 0 on a stop cell): one thread per row.
__global__ __launch_bounds__(256) void rc_build_runs_kernel(RcTrackDev t, uint8_t *__restrict__ run_neg, uint8_t *__restrict__ run_pos) {
    const int iy = blockIdx.x * blockDim.x + threadIdx.x;
    if (iy >= t.h) return;
    int r = 0;
    for (int ix = 0; ix < t.w; ++ix) {                          // towards -x: cells ix, ix - 1, ... are free
        r = bit_at(t.ray_words, t.pitch, ix, iy) ? 0 : min(r + 1, 255);
        run_neg[(size_t)iy * t.w + ix] = (uint8_t)r;
    }
    r = 0;
    for (int ix = t.w - 1; ix >= 0; --ix) {
        r = bit_at(t.ray_words, t.pitch, ix, iy) ? 0 : min(r + 1, 255);
        run_pos[(size_t)iy * t.w + ix] = (uint8_t)r;
    }
}

// One thread per (cell, quadrant): among the free rectangles anchored at the cell (width = min over its rows of the free
// run towards sx) the one with the largest geometric mean of the exit distances of rays at 11.25, 33.75, 56.25 and
// 78.75 degrees inside the quadrant.
__global__ __launch_bounds__(256) void rc_build_quad_kernel(RcTrackDev t, const uint8_t *__restrict__ run_neg,
                                                            const uint8_t *__restrict__ run_pos, uint16_t *__restrict__ out) {
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (unsigned)t.h * (unsigned)t.w * 4u) return;
    const int q = (int)(gid & 3u);
    const unsigned cell = gid >> 2;
    const int ix = (int)(cell % (unsigned)t.w), iy = (int)(cell / (unsigned)t.w);
    const int sx = (q & 1) ? -1 : 1, sy = (q & 2) ? -1 : 1;       // plane q = (dy < 0) * 2 + (dx < 0)
    // mirrored storage: a ray heading -x reads its plane with the columns reversed (likewise -y and the rows)
    const int rx = sx > 0 ? ix : t.w - 1 - ix, ry = sy > 0 ? iy : t.h - 1 - iy;
    uint16_t &e = out[(size_t)q * (t.quad_plane_bytes / 2) + (size_t)ry * t.cell_pitch + rx];
    if (ix == 0 || iy == 0 || ix == t.w - 1 || iy == t.h - 1) { e = 0x0100; return; }       // sentinel ring: "no return"
    if (bit_at(t.ray_words, t.pitch, ix, iy)) { e = 0; return; }                              // wall
    const uint8_t *run = sx > 0 ? run_pos : run_neg;
    // 1 / cos and 1 / sin of the four sample directions
    const float ka[4] = {1.0195911f, 1.2026898f, 1.7999525f, 5.1258309f};
    const float kb[4] = {5.1258309f, 1.7999525f, 1.2026898f, 1.0195911f};
    const float log_ka_sum = __logf(ka[0]) + __logf(ka[1]) + __logf(ka[2]) + __logf(ka[3]);
    int cur = 255, bw = 1, bh = 1;
    float best = -1.0e30f;
    for (int n = 1; n <= 255; ++n) {
        const int y = iy + (n - 1) * sy;
        if (y < 0 || y >= t.h) break;
        cur = min(cur, (int)run[(size_t)y * t.w + ix]);
        // the width only shrinks from here on and the score is at most sum log(width * ka)
        if (cur == 0 || 4.0f * __logf((float)cur) + log_ka_sum <= best) break;
        float sc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) sc += __logf(fminf((float)cur * ka[k], (float)n * kb[k]));
        if (sc > best) { best = sc; bw = cur; bh = n; }
    }
    e = (uint16_t)(bw | (bh << 8));
}

}  // namespace

hipError_t rck_build_quad_planes(const RcTrackDev &t, uint16_t *quad_rect_dev, hipStream_t s) {
    uint8_t *runs = nullptr;
    const size_t plane = (size_t)t.h * t.w;
    hipError_t e = hipMalloc((void **)&runs, 2 * plane);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rc_build_runs_kernel, dim3((unsigned)((t.h + 255) / 256)), dim3(256), 0, s, t, runs, runs + plane);
    const long long total = (long long)plane * 4;
    hipLaunchKernelGGL(rc_build_quad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t, runs, runs + plane, quad_rect_dev);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(runs);
    return e;
}

hipError_t rck_build_spawn_table(const RcTrackDev &t, float4 *spawn_dev, hipStream_t s) {
    hipLaunchKernelGGL(rc_build_spawn_kernel, dim3((t.n_centerline + 255) / 256), dim3(256), 0, s, t, spawn_dev);
    return hipGetLastError();
}

hipError_t rck_build_first_table(const RcTrackDev &t, uint16_t *first_rect_dev, hipStream_t s) {
    RcFirstBin bins[RC_FIRST_BINS];
    // bin b = the float bits of the slope >> RC_FIRST_SHIFT, less RC_FIRST_BIAS: exponent -4 + b / 8 and the top three
    // mantissa bits b % 8, i.e. the slopes [2^e (1 + m / 8), 2^e (1 + (m + 1) / 8)) - eight LINEAR steps per octave
    constexpr int kPerOctave = RC_FIRST_BINS / 8, kMantBits = 23 - RC_FIRST_SHIFT;
    static_assert((1 << kMantBits) == kPerOctave && RC_FIRST_BIAS == (123u << kMantBits), "bins = exponent and top mantissa bits over 2^-4 .. 2^4");
    auto edge = [](int b) { return std::exp2(-4.0 + (double)(b / kPerOctave)) * (1.0 + (double)(b % kPerOctave) / kPerOctave); };
    for (int b = 0; b < RC_FIRST_BINS; ++b) {
        const double lo = edge(b), hi = edge(b + 1);                 // slope |dy / dx| of the bin
        const bool swap = b >= RC_FIRST_BINS / 2;
        // slope range in the bin's own frame, widened by 1e-6; the outermost bins are open-ended
        const double e1 = swap ? 1.0 / hi : lo, e2 = swap ? 1.0 / lo : hi;
        bins[b].s1 = (b == 0 || b == RC_FIRST_BINS - 1) ? 0.0f : (float)(e1 * (1.0 - 1e-6));
        bins[b].s2 = (float)(e2 * (1.0 + 1e-6));
        for (int k = 0; k < 2; ++k) {
            const double ang = std::atan(lo + (hi - lo) * (k ? 0.75 : 0.25));
            (k ? bins[b].ka1 : bins[b].ka0) = (float)(1.0 / std::cos(ang));
            (k ? bins[b].kb1 : bins[b].kb0) = (float)(1.0 / std::sin(ang));
        }
    }
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_first_bins), bins, sizeof(bins));
    if (e != hipSuccess) return e;
    const long long total = (long long)t.h * t.w * RC_FIRST_PLANES;
    if (total >= (1LL << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rc_build_first_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t, first_rect_dev);
    return hipGetLastError();
}


// Validation of a freshly built track's tables (rc_load_track): the BOUNDED build of the default scan from every cell a
// sensor can stand in - the centre of every non-stop cell, two opposite headings, so that all 4 x 64 first-trip entries of
// the cell and both signs of every direction are used - with no output kept.  A ray that uses up its trip budget (a table
// entry that sends it in circles or off the grid's ring) is counted; the caller refuses the track if any did.
__global__ __launch_bounds__(256) void rc_validation_poses_kernel(RcTrackDev t, float4 *__restrict__ poses, uint32_t *__restrict__ count) {
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (unsigned)t.h * (unsigned)t.w) return;
    const int ix = (int)(gid % (unsigned)t.w), iy = (int)(gid / (unsigned)t.w);
    if (bit_at(t.ray_words, t.pitch, ix, iy)) return;                     // stop cell (wall or ring): no sensor scans from here
    const float cx = t.org_x + ((float)ix + 0.5f) * t.res, cy = t.org_y + ((float)iy + 0.5f) * t.res;
    float sn, cs;
    sincos32(0.3f, sn, cs);
    const unsigned k = atomicAdd(count, 2u);
    poses[k] = make_float4(cx - RCS_LIDAR_X * cs, cy - RCS_LIDAR_X * sn, cs, sn);          // sensor at the cell's centre
    poses[k + 1] = make_float4(cx + RCS_LIDAR_X * cs, cy + RCS_LIDAR_X * sn, -cs, -sn);
}

hipError_t rck_validate_tables(const RcTrackDev &t, float band, hipStream_t s, unsigned long long *n_scans, unsigned *n_overruns) {
    const size_t cells = (size_t)t.h * t.w;
    float4 *poses = nullptr;
    uint32_t *counters = nullptr, host[2] = {0u, 0u};
    hipError_t e = hipMalloc((void **)&poses, 2 * cells * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void **)&counters, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * sizeof(uint32_t), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rc_validation_poses_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, t, poses, counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, counters, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && host[0] != 0u) {
        RcParams p{};
        p.trk = t;
        p.trk.band = band; p.trk.band_mh = band - 0.5f; p.trk.band2 = 2.0f * band;
        p.st.scan_pose = poses;
        p.num_envs = p.n_cars = (int32_t)host[0];
        p.cars_per_env = 1;
        p.scan_overrun = counters + 1;
        RcLaunchInfo li{};                  // rc_raycast_car_kernel<1, false, true>, one car per 64-thread workgroup
        li.raycast_variant = 7; li.car_threads = 64; li.car_split = 1; li.scan_guarded = 1;
        e = rck_launch_raycast(p, li, nullptr, s);
        if (e == hipSuccess) e = hipMemcpyAsync(host, counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (poses) (void)hipFree(poses);
    if (counters) (void)hipFree(counters);
    *n_scans = host[0];
    *n_overruns = host[1];
    return e;
}
