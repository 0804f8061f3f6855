// The two follow-the-gap agents on the device (rc_follow_the_gap, rc_follow_the_gap_reference): kernels, launchers, entry points.
#include "racecar_scan.h"
#include "racecar_env.h"

namespace {

// Follow-the-gap on the device: one wave per car, lane l owns the 13 consecutive beams FTG_LO + 13 l ...
// Wave-level steps use shuffles only: (value, index) arg-min for the closest return, and an ordered
// tree reduction of run summaries (leading / trailing / best run of gap beams) for the widest gap.
#define FTG_LO 135
#define FTG_N 810
#define FTG_PER_LANE 13
#define FTG_BUBBLE 60
#define FTG_GAP_RANGE 2.0f      // a beam belongs to a gap if its smoothed range exceeds this [m]
#define FTG_CLIP 6.0f           // ranges are clipped here first (with the 0.19 rad lock the car must see a corner early)

struct RunSummary { int len, pre, suf, best, bstart, all; };

__device__ __forceinline__ RunSummary run_combine(const RunSummary &a, const RunSummary &b, int a_end) {
    // a covers [.., a_end), b starts at a_end; ties keep the earlier run
    RunSummary r;
    r.len = a.len + b.len;
    r.all = a.all & b.all;
    r.pre = a.all ? a.len + b.pre : a.pre;
    r.suf = b.all ? b.len + a.suf : b.suf;
    const int cross = a.suf + b.pre, cstart = a_end - a.suf;
    r.best = a.best; r.bstart = a.bstart;
    if (cross > r.best) { r.best = cross; r.bstart = cstart; }
    if (b.best > r.best) { r.best = b.best; r.bstart = b.bstart; }
    return r;
}

__global__ __launch_bounds__(256) void rc_ftg_kernel(RcParams p, float *__restrict__ actions, float motor_straight,
                                                      float motor_corner) {
    const int lane = threadIdx.x & 63;
    const int car = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (car >= p.n_cars) return;
    const float *scan = p.out.lidar + (size_t)car * RC_N_BEAMS;
    const int e0 = lane * FTG_PER_LANE;                              // first element (relative to FTG_LO)
    // The arc goes through LDS: read from memory with consecutive lanes on consecutive beams (256-byte requests; a lane
    // reading its own 17 beams directly makes every load touch 52 lines), clipped, then each lane takes its 13 beams
    // plus a halo of 2 on each side (stride 13 dwords: conflict-free).  Slots -2, -1 and >= FTG_N are zero padding.
    __shared__ float arc[4][FTG_PER_LANE * 64 + 8];
    float *row = arc[threadIdx.x >> 6] + 2;
#pragma unroll
    for (int k = 0; k < FTG_PER_LANE; ++k) {
        const int e = lane + 64 * k;
        float v = 0.0f;
        if (e < FTG_N) {
            v = scan[FTG_LO + e];
            v = v > FTG_CLIP ? FTG_CLIP : v;
        }
        row[e] = v;
    }
    if (lane < 2) { row[lane - 2] = 0.0f; row[FTG_PER_LANE * 64 + lane] = 0.0f; }
    __builtin_amdgcn_wave_barrier();                                 // one wave per car: its own LDS writes, in order
    float r[FTG_PER_LANE + 4];
#pragma unroll
    for (int k = 0; k < FTG_PER_LANE + 4; ++k) r[k] = row[e0 + k - 2];
    float sm[FTG_PER_LANE];
    float best_v = INFINITY;
    int best_i = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < FTG_PER_LANE; ++k) {
        const int e = e0 + k;
        sm[k] = ((((r[k] + r[k + 1]) + r[k + 2]) + r[k + 3]) + r[k + 4]) * 0.2f;
        if (e < FTG_N && sm[k] < best_v) { best_v = sm[k]; best_i = e; }
    }
    // closest return: wave arg-min, first index wins ties
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best_v, off);
        const int oi = __shfl_xor(best_i, off);
        if (ov < best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
    }
    const int closest = best_i;
    // gap beams: positive after the bubble; summarise this lane's 13 beams
    RunSummary s;
    s.len = 0; s.pre = 0; s.suf = 0; s.best = 0; s.bstart = e0; s.all = 1;
    int run = 0;
#pragma unroll
    for (int k = 0; k < FTG_PER_LANE; ++k) {
        const int e = e0 + k;
        const bool inside = e < FTG_N;
        const bool gap = inside && sm[k] > FTG_GAP_RANGE && (e < closest - FTG_BUBBLE || e > closest + FTG_BUBBLE);
        if (inside) {
            s.len += 1;
            if (gap) {
                run += 1;
                if (run > s.best) { s.best = run; s.bstart = e - run + 1; }
            } else {
                if (s.all) s.pre = run;
                s.all = 0;
                run = 0;
            }
        }
    }
    if (s.all) s.pre = run;
    s.suf = run;
    // ordered tree reduction: lane i absorbs lane i + off
    int my_end = e0 + s.len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        RunSummary o;
        o.len = __shfl_down(s.len, off); o.pre = __shfl_down(s.pre, off); o.suf = __shfl_down(s.suf, off);
        o.best = __shfl_down(s.best, off); o.bstart = __shfl_down(s.bstart, off); o.all = __shfl_down(s.all, off);
        if ((lane & (2 * off - 1)) == 0 && lane + off < 64) {
            s = run_combine(s, o, my_end);
            my_end += o.len;
        }
    }
    if (lane == 0) {
        float motor = 0.0f, steering = 0.0f;
        if (s.best > 0) {
            const float centre = (float)FTG_LO + ((float)(2 * s.bstart + s.best - 1)) * 0.5f;
            const float angle = 2.35619449019234492885f - centre * 0.00436737625568553f;   // 135 deg - i * 270/1079 deg
            steering = clampf(angle / RCS_STEER_GAIN, -1.0f, 1.0f);          // the command that points the wheels at the gap (+ = right)
            motor = fabsf(steering) > 0.35f ? motor_corner : motor_straight;
        }
        actions[2 * car] = motor;
        actions[2 * car + 1] = steering;
    }
}

// ---- The REFERENCE's follow-the-gap law on the device (ros_agent/agents/follow_the_gap/src/agent.py:128-234 of the
// reference: disparity extender + percentile heading + P/D steering) - oracle/racecar_oracle.py, follow_the_gap_reference,
// is the binary32 spec this kernel follows operation for operation; oracle/ftg_reference_port.py restates the node in
// float64 and tests/golden/ftg_golden.npz pins both to the node's own outputs.  One wave per car; arc element
// a = ROS beam 179 + a = this build's beam 900 - a, 721 of them, lane l holds a = l + 64 k.
#define FR_FIRST 179
#define FR_N 721
#define FR_HALF 19                      // the 10-degree filter: 39 beams
#define FR_PER_LANE 12
// (binary32 values of the oracle's float64 expressions, as hexadecimal literals: no decimal rounding in between)
constexpr float kFrInc = 0x1.1e3842p-8f;                 // fp32(1.5 pi / 1079) = 0.004367367
constexpr float kFrAmin = -0x1.2d97c8p+1f;               // fp32(-0.75 pi)
constexpr float kFrLookahead = 0x1.7ba938p+2f;           // fp32(2 x 7^2 / (2 x 8.26)) = 5.9322033
constexpr float kFrW2 = 0x1.418c7p-3f;                   // fp32((1.2 x 0.3302)^2) = 0.15700614
constexpr float kFrMaxSteer = 0x1.aceeap-2f;             // fp32(24 deg)
constexpr float kFrDeg5 = 0x1.657184p-4f;                // fp32(5 deg)

__device__ __forceinline__ float fr_asin_small(float t) {            // |t| <= 0.5 (cephes asinf)
    const float z = t * t;
    const float pz = ((((4.2163199048e-2f * z + 2.4181311049e-2f) * z + 4.5470025998e-2f) * z + 7.4953002686e-2f) * z + 1.6666752422e-1f) * z;
    return pz * t + t;
}
// Correctly rounded binary32 square root (racecar_device.h, rcd::sqrt_rn: what the spec's np.sqrt is)
__device__ __forceinline__ float fr_sqrt_rn(float x) { return rcd::sqrt_rn(x); }
// Device self-test of that (rc_selftest_sqrt): every binary32 in [lo_bits, hi_bits] against the double-precision root rounded once
__global__ __launch_bounds__(256) void rc_selftest_sqrt_kernel(uint32_t lo_bits, uint32_t hi_bits, unsigned long long *mismatches) {
    unsigned long long bad = 0;
    for (uint64_t b = (uint64_t)lo_bits + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; b <= hi_bits; b += (uint64_t)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t)b);
        bad += __float_as_uint(fr_sqrt_rn(x)) != __float_as_uint((float)sqrt((double)x));
    }
    if (bad) atomicAdd(mismatches, bad);
}

__device__ __forceinline__ float fr_acos(float x) {                  // racecar_oracle.acos32
    const float ax = fabsf(x);
    if (!(ax <= 1.0f)) return __builtin_nanf("");
    if (ax > 0.5f) {
        const float a = 2.0f * fr_asin_small(fr_sqrt_rn((1.0f - ax) * 0.5f));
        return x < 0.0f ? 3.14159274101257324f - a : a;
    }
    return 1.57079637050628662f - fr_asin_small(x);
}
__device__ __forceinline__ float fr_angle(int a) { return (float)(FR_FIRST + a) * kFrInc + kFrAmin; }
__device__ __forceinline__ int wave_count(bool c) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(c)); }
// Reductions over the 64 lanes on the DPP paths of the vector unit (one instruction per step, no LDS crossbar): within rows of
// 16 by quad permutes and mirrors, then lane 15 of a row into the next (row_bcast:15, rows 1 and 3) and lane 31 into the upper
// half (row_bcast:31); lane 63 holds the result.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_pull(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xF, false); }
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op) {
    v = op(v, dpp_pull<0xB1, 0xF>(v));       // quad_perm:[1,0,3,2]
    v = op(v, dpp_pull<0x4E, 0xF>(v));       // quad_perm:[2,3,0,1]
    v = op(v, dpp_pull<0x141, 0xF>(v));      // row_half_mirror
    v = op(v, dpp_pull<0x140, 0xF>(v));      // row_mirror: every lane of a row holds the row's result
    const uint32_t r1 = dpp_pull<0x142, 0xA>(v);     // (rows not named keep their own value: see the selects)
    v = (__lane_id() & 16) ? op(v, r1) : v;
    const uint32_t r2 = dpp_pull<0x143, 0xC>(v);
    v = (__lane_id() & 32) ? op(v, r2) : v;
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; }); }

__global__ __launch_bounds__(256) void rc_ftg_reference_kernel(RcParams p, float *__restrict__ actions, float *__restrict__ prev_heading,
                                                               float dt, float *__restrict__ detail) {
    const int lane = threadIdx.x & 63;
    const int car = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (car >= p.n_cars) return;
    // Two arrays of 832 floats per wave (6.6 KB: six waves per SIMD).  `ra`: the clipped arc r[a] - overwritten by the window
    // maxima while they are built, written again from registers afterwards; `jp`: the jumps with 19 mirrored values on each
    // side (jp[i] = jump[i - 19]), kept to the end.  Both end in zeros (reads beyond the data).
    constexpr int kBuf = FR_PER_LANE * 64 + 64;
    __shared__ float lds_a[4][kBuf], lds_b[4][kBuf];
    float *ra = lds_a[threadIdx.x >> 6], *jp = lds_b[threadIdx.x >> 6];
    const float *scan = p.out.lidar + (size_t)car * RC_N_BEAMS;
    // the arc, clipped at the look-ahead distance (agent.py:141-146); consecutive lanes read consecutive beams
    float rv[FR_PER_LANE];
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int a = lane + 64 * k;
        float v = 0.0f;
        if (a < FR_N) {
            v = scan[900 - a];
            v = v > 0.0f ? v : 0.0f;                                 // (also turns a NaN into 0)
            v = v < kFrLookahead ? v : kFrLookahead;
        }
        rv[k] = v;
        ra[a] = v;
    }
    ra[FR_PER_LANE * 64 + lane] = 0.0f;
    jp[kBuf - 128 + lane] = 0.0f;                                    // [704, 768) - the jumps below overwrite what they own -
    jp[kBuf - 64 + lane] = 0.0f;                                     // and [768, 832)
    __builtin_amdgcn_wave_barrier();
    // (758 padded values: 720 jumps + 2 x 19)
    float jv[FR_PER_LANE];
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int a = lane + 64 * k;
        jv[k] = a < FR_N - 1 ? fabsf(ra[a + 1] - rv[k]) : 0.0f;     // agent.py:148
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int a = lane + 64 * k;
        if (a < FR_N - 1) jp[a + FR_HALF] = jv[k];
        if (k == 0 && a < FR_HALF) jp[FR_HALF - 1 - a] = jv[k];                                  // scipy's 'reflect' border
        if (k >= 10 && a >= FR_N - 1 - FR_HALF && a < FR_N - 1) jp[2 * (FR_N - 1) - 1 - a + FR_HALF] = jv[k];
    }
    __builtin_amdgcn_wave_barrier();
    // The maximum of every 39-beam window (agent.py:154) by doubling: windows of 2, 4, 8, 16, 32 - each pass one neighbour read
    // and one maximum per element, in place in `ra` (all reads of a pass before its writes) - and 39 = 32 and 32 seven further
    // on.  The window of beam a is padded [a, a + 38].
    // (jumps are >= +0 and never NaN: their bit patterns order like the values, and an integer maximum is ONE instruction
    // where the floating-point select is a compare and a move)
    uint32_t *rau = reinterpret_cast<uint32_t *>(ra);
    const uint32_t *jpu = reinterpret_cast<const uint32_t *>(jp);
    uint32_t w[FR_PER_LANE], o[FR_PER_LANE];
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        const uint32_t x = jpu[i], y = jpu[i + 1];
        w[k] = y > x ? y : x;
    }
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) rau[lane + 64 * k] = w[k];
#pragma unroll
    for (int sft = 2; sft <= 16; sft <<= 1) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < FR_PER_LANE; ++k) o[k] = rau[lane + 64 * k + sft];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < FR_PER_LANE; ++k) {
            w[k] = o[k] > w[k] ? o[k] : w[k];
            rau[lane + 64 * k] = w[k];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // candidates (agent.py:150-156): a jump that is the maximum of its window and exceeds 0.2 m; bit k of `cbits` = this
    // lane's element k is one
    uint32_t cbits = 0u;
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int a = lane + 64 * k;
        const uint32_t x = rau[a + 7];
        const uint32_t peak = x > w[k] ? x : w[k];                    // windows [a, a + 31] and [a + 7, a + 38] of the padded array
        if (a < FR_N - 1 && __float_as_uint(jv[k]) == peak && jv[k] > 0.2f) cbits |= 1u << k;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) ra[lane + 64 * k] = rv[k];  // the arc again (rv[] becomes the adjusted arc below)
    __builtin_amdgcn_wave_barrier();
    // One candidate at a time, the wave together (their order does not matter: the extension is a minimum).  A candidate is a
    // disparity if it exceeds nine times the MEDIAN of its window (agent.py:157-159, ends repeated) - and since x -> fl(9 x) is
    // monotone, "jump > 9 median" holds exactly when at least 20 of the 39 samples satisfy "jump > 9 sample": no sorting.
    unsigned long long todo = __builtin_amdgcn_ballot_w64(cbits != 0u);
    while (todo != 0) {
        const int l = __builtin_ctzll(todo);
        const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)cbits, l);
        const int ac = l + 64 * __builtin_ctz(bits);                  // wave-uniform
        if (lane == l) cbits &= cbits - 1u;
        if ((bits & (bits - 1u)) == 0u) todo &= todo - 1;
        int i = ac - FR_HALF + lane;
        i = i < 0 ? 0 : (i > FR_N - 2 ? FR_N - 2 : i);
        const float mine = jp[i + FR_HALF];
        const float jc = jp[ac + FR_HALF];
        if (wave_count(lane <= 2 * FR_HALF && jc > mine * 9.0f) <= FR_HALF) continue;
        // extend the nearer side by the half-width of the vehicle as seen at that range (agent.py:165-176)
        const float near = fminf(fminf(ra[ac > 0 ? ac - 1 : 0], ra[ac]), ra[ac + 1]);
        const float two = 2.0f * (near * near);
        const float half = fr_acos((two - kFrW2) / two);
        int ia = 0, ib = 0;
        if (half == half) {
            const float a0 = fr_angle(0), at = fr_angle(ac);
            const float lo = ((at - half) - a0) / kFrInc, hi = ((at + half) - a0) / kFrInc;
            ia = (int)lo; ib = (int)hi;
            ia = ia < 0 ? 0 : (ia > FR_N - 1 ? FR_N - 1 : ia);
            ib = ib < 0 ? 0 : (ib > FR_N - 1 ? FR_N - 1 : ib);
        }
#pragma unroll
        for (int e = 0; e < FR_PER_LANE; ++e) {
            const int a = lane + 64 * e;
            if (a >= ia && a <= ib) rv[e] = __uint_as_float(min(__float_as_uint(rv[e]), __float_as_uint(near)));      // (both >= +0)
        }
    }
    float adj[FR_PER_LANE];
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) adj[k] = lane + 64 * k < FR_N ? rv[k] : INFINITY;   // (slots beyond the arc: above every rank)
    // the 601st and 602nd smallest adjusted range (agent.py:183, np.percentile at q = 83.3): ranges are >= 0, so their
    // bit patterns order like the values; binary search on the pattern, counts by ballot.  [lo, lo + 2^bit) always holds
    // the wanted key (c_lo keys below it, c_hi below its end, c_lo <= 600 < c_hi): once it holds ONE key the search is
    // over - about half way for a scan's spread of ranges; ties run to the last bit.
    uint32_t key[FR_PER_LANE];
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) key[k] = __float_as_uint(adj[k]);
    uint32_t x600 = 0u;
    int c_lo = 0, c_hi = FR_PER_LANE * 64, bit = 30;
    for (; bit >= 0; --bit) {
        const uint32_t trial = x600 | (1u << bit);
        int below = 0;
#pragma unroll
        for (int k = 0; k < FR_PER_LANE; ++k) below += wave_count(key[k] < trial);
        if (below <= 600) { x600 = trial; c_lo = below; } else c_hi = below;
        if (c_hi - c_lo == 1) break;
    }
    if (bit >= 0) {                                                   // the one key at or above the bucket's start
        uint32_t only = 0xffffffffu;
#pragma unroll
        for (int k = 0; k < FR_PER_LANE; ++k) only = key[k] >= x600 && key[k] < only ? key[k] : only;
        x600 = wave_min_u32(only);
    }
    int not_above = 0;
    uint32_t next = 0x7f800000u;
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        not_above += wave_count(key[k] <= x600);
        if (key[k] > x600 && key[k] < next) next = key[k];
    }
    const uint32_t x601 = not_above >= 602 ? x600 : wave_min_u32(next);
    // NumPy's linear interpolation at virtual index 600.0000000000001: a + (b - a) * 2^-43 in binary64; a binary32 range is
    // at or above that threshold exactly when it is at or above the threshold rounded UP to binary32
    const double a64 = (double)__uint_as_float(x600), b64 = (double)__uint_as_float(x601);
    const double thr = a64 + (b64 - a64) * 1.1368683772161603e-13;
    float thr32 = (float)thr;
    if ((double)thr32 < thr) thr32 = __uint_as_float(__float_as_uint(thr32) + 1u);      // (thr >= 0 and finite)
    int count = 0;
    uint32_t sum_k = 0u, sum_q = 0u;
#pragma unroll
    for (int k = 0; k < FR_PER_LANE; ++k) {
        const int a = lane + 64 * k;
        const bool chosen = a < FR_N && adj[k] >= thr32 && adj[k] < RCS_MAX_RANGE;           // np.digitize(...) == 2
        count += wave_count(chosen);
        sum_k += chosen ? (uint32_t)a : 0u;
        sum_q += chosen ? (uint32_t)__builtin_rintf(ra[a] * 524288.0f) : 0u;
    }
    sum_k = wave_sum_u32(sum_k);
    sum_q = wave_sum_u32(sum_q);
    if (lane == 0) {
        const float cnt = (float)count;
        const float heading = (((float)(int)sum_k / cnt) + (float)FR_FIRST) * kFrInc + kFrAmin;          // agent.py:184
        const float hd = ((float)sum_q / cnt) * (1.0f / 524288.0f);                                 // agent.py:185
        // agent.py:200-234 with PID.calculate (kp 1.4, kd 0.1): no derivative term on an episode's first command
        const float prev = p.st.fresh[car] ? __builtin_nanf("") : prev_heading[car];
        const float d_term = prev == prev ? (0.1f * (prev - heading)) / dt : 0.0f;
        float steer = 1.4f * heading - d_term;
        steer = steer > -kFrMaxSteer ? steer : -kFrMaxSteer;
        steer = steer < kFrMaxSteer ? steer : kFrMaxSteer;
        float speed = fabsf(steer) > kFrDeg5 ? 6.0f - (fabsf(steer) / kFrMaxSteer) * 1.8f : 6.0f;
        if (hd < 5.0f) { const float lim = (hd / 5.0f) * 4.0f; speed = lim < speed ? lim : speed; }
        speed = speed > 1.5f ? speed : 1.5f;
        prev_heading[car] = heading;
        // the car's actuators: target speed over its top speed, steering angle over its steering limit
        float motor = clampf(speed / RCS_MAX_VEL, -1.0f, 1.0f), steering = clampf(steer / RCS_STEER_GAIN, -1.0f, 1.0f);
        if (p.remap_actions) {                 // the caller's convention is ReduceActionSpace's (wrappers.py:128-130): invert it
            motor = ((motor - p.act_lo0) * 2.0f) / (p.act_hi0 - p.act_lo0) - 1.0f;
            steering = ((steering - p.act_lo1) * 2.0f) / (p.act_hi1 - p.act_lo1) - 1.0f;
        }
        actions[2 * car] = motor;
        actions[2 * car + 1] = steering;
        if (detail != nullptr) {
            detail[4 * car] = heading; detail[4 * car + 1] = hd; detail[4 * car + 2] = steer; detail[4 * car + 3] = speed;
        }
    }
}

}  // namespace

hipError_t rck_launch_ftg(const RcParams &p, float *actions, float motor_straight, float motor_corner, hipStream_t s) {
    const int threads = 256, blocks = (p.n_cars + 3) / 4;
    launch(rc_ftg_kernel, dim3(blocks), dim3(threads), 0, s, p, actions, motor_straight, motor_corner);
    return hipGetLastError();
}

hipError_t rck_launch_ftg_reference(const RcParams &p, float *actions, float *prev_heading, float dt, float *detail, hipStream_t s) {
    const int threads = 256, blocks = (p.n_cars + 3) / 4;
    launch(rc_ftg_reference_kernel, dim3(blocks), dim3(threads), 0, s, p, actions, prev_heading, dt, detail);
    return hipGetLastError();
}

hipError_t rck_launch_selftest_sqrt(uint32_t lo_bits, uint32_t hi_bits, unsigned long long *mismatches_dev, hipStream_t s) {
    hipLaunchKernelGGL(rc_selftest_sqrt_kernel, dim3(4096), dim3(256), 0, s, lo_bits, hi_bits, mismatches_dev);
    return hipGetLastError();
}

extern "C" {

int rc_follow_the_gap(rc_env *env, float motor_straight, float motor_corner) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->was_reset) return fail(RC_ERR_NEEDS_RESET, "Must reset environment.");
    HIP_TRY(hipSetDevice(env->cfg.device));
    TIMED(env, RC_K_FTG, rck_launch_ftg(env->params, env->actions_in, motor_straight, motor_corner, env->stream));
    return RC_OK;
}

int rc_follow_the_gap_reference(rc_env *env, float dt, float *detail_dev) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->was_reset) return fail(RC_ERR_NEEDS_RESET, "Must reset environment.");
    if (!(dt > 0.f)) return fail(RC_ERR_INVALID, "dt must be > 0 (seconds per agent step)");
    if (env->cfg.lidar_transform != RC_LIDAR_METRES) return fail(RC_ERR_INVALID, "rc_follow_the_gap_reference reads the scan in metres (lidar_transform RC_LIDAR_METRES)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    if (!env->ftg_prev) {
        HIP_TRY(hipMalloc((void **)&env->ftg_prev, (size_t)env->n_cars * sizeof(float)));
        HIP_TRY(hipMemsetAsync(env->ftg_prev, 0xff, (size_t)env->n_cars * sizeof(float), env->stream));      // all ones: a NaN
    }
    TIMED(env, RC_K_FTG, rck_launch_ftg_reference(env->params, env->actions_in, env->ftg_prev, dt, detail_dev, env->stream));
    return RC_OK;
}

}  // extern "C"
