// rc_policy_decode_lidar: the reference's LidarDistanceDecoder (dreamer/models.py:424-441) from a feature [stoch 30 | deter 200] -
// a car's stored latent or a row of rc_policy_imagine's / rc_policy_observe's features - to the IndependentNormal over the 1080
// beams in the model's units (scan_m / 15 - 0.5): loc, scale = softplus(raw) and, against a target scan, the log-probability, in
// the binary32 arithmetic of DESIGN.md §2 item 22 (tests/policy_lidar_decode_spec.c is the CPU restatement): dense1 230 -> 256
// (no activation), dense2 256 -> 512 (ReLU), params 512 -> 2160 (leaky ReLU, slope 0.2).  An output of dense1 and dense2 is one
// fmaf chain from its bias, k ascending, as everywhere in the agent.  An output of params is the chain from +0.0f, the bias added
// LAST: the raw-scale columns of a narrow decoder carry a bias near -30 (scale = softplus(0.2 x that) = 2.5e-3), and a chain that
// started there would round each of its 512 steps at that magnitude - 13 ulp of the pre-activation, 46 ulp of the scale, measured
// on the spec - where one final addition rounds once.
//
// One workgroup of four waves owns 32 rows (racecar_policy_tiles.h).  LDS: A [32][513] holds the features, then dense2's output;
// B [32][257] holds dense1's output; 101 KB with the partial sums below, so one workgroup per CU (dense2's 512 columns and
// dense1's 256 are alive at the same time: two workgroups would need both below 80 KB).  The last layer never leaves the
// registers: a wave takes the output tiles in PAIRS, columns {32 j, 1088 + 32 j} of the device image, so that a lane's
// accumulator registers hold loc and raw scale of the same (row, beam), and mean, std and the log-likelihood term are formed
// there - the 2160 pre-activations of a row are written nowhere.
//
// The partial tile.  1080 = 33 x 32 + 24: in the checkpoint's [512][2160] array the 34th loc tile would run 8 columns into the
// scale columns and the 34th scale tile 8 columns past the end of the array.  The device copy is PADDED, not clamped: params_w /
// params_b are repacked (rc_policy_load_lidar_decoder) as loc columns [0, 1080), zeros [1080, 1088), scale columns
// [1088, 2168), zeros [2168, 2176), ld = 2176 = 68 tiles, so every tile of every pair lies inside the image and the eight
// lanes 24 - 31 of pair 33 compute 0 from zero weights and a zero bias.  They are masked out of every store and enter the
// log-likelihood's sum as +0.0f terms, which the spec's sum holds at the same places.
//
// The log-likelihood's order of summation (fixed by the spec, the same for every launch shape): within pair j the 32 terms of
// a row are added in a binary tree over the beam's index (distance 1, 2, 4, 8, 16: the butterfly below computes exactly that
// tree in lane 0, addition being commutative), giving 34 partial sums per row; they are added in ascending j from +0.0f.
#include "racecar_env.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int LFEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
constexpr int LBEAMS = RC_LDEC_BEAMS;
constexpr int LAS = RC_LDEC_H2 + 1;            // row stride of A (513: odd, the 32 rows on 32 banks)
constexpr int LBS = RC_LDEC_H1 + 1;            // row stride of B (257)
constexpr int LPAIRS = (LBEAMS + 31) / 32;     // 34 tile pairs, the last one 24 beams wide
constexpr int LPS = LPAIRS + 1;                // row stride of the partial sums (35)
constexpr int O_LA = 0, O_LB = O_LA + PM * LAS, O_LP = O_LB + PM * LBS, N_LLDS = O_LP + PM * LPS;
constexpr size_t kLidarLdsBytes = (size_t)N_LLDS * sizeof(float);
static_assert(kLidarLdsBytes <= 160 * 1024, "the workgroup's LDS must fit a CU");
static_assert(LFEAT % 2 == 0 && RC_LDEC_H1 % 2 == 0 && RC_LDEC_H2 % 2 == 0, "k-steps of 2");
static_assert(RC_LDEC_H1 == 8 * 32 && RC_LDEC_H2 == 16 * 32, "dense1: 2 tiles per wave, dense2: 4");
static_assert(LPAIRS % 2 == 0 && RC_LDEC_HALF >= 32 * LPAIRS && RC_LDEC_LD == 2 * RC_LDEC_HALF, "pairs of pairs; every tile inside the padded image");
static_assert(LFEAT <= RC_LDEC_H2, "the features lie where dense2's output goes");

__device__ __forceinline__ float ld_leaky(float v) { return v > 0.0f ? v : 0.2f * v; }

// The epilogue of pair p on the accumulators of its loc and scale tiles
__device__ __forceinline__ void ld_pair(const RcLidarDecodeCall &c, const pm_f32x16 &aloc, const pm_f32x16 &araw, int p, int64_t row0, int lane,
                                        float *part) {
    const int cc = lane & 31, half = lane >> 5;
    const int beam = 32 * p + cc;
    const float b_loc = c.w.p_b[beam], b_raw = c.w.p_b[RC_LDEC_HALF + beam];      // (inside the padded image for every lane)
    const bool live = beam < LBEAMS;                       // (pair 33: lanes 24 - 31 are padding)
    const bool want_sd = c.std || c.loglik;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = pm_row(r, half);
        const int64_t q = row0 + row;
        int64_t at = -1;
        if (q < c.n_rows) at = c.features ? q : (int64_t)pm_car(c.rows, (int)q);
        const bool store = live && at >= 0;
        const float loc = ld_leaky(aloc[r] + b_loc);
        float term = 0.0f;
        if (store && c.mean) c.mean[(size_t)at * LBEAMS + beam] = loc;
        if (want_sd) {
            const float sd = pm_softplus(ld_leaky(araw[r] + b_raw));
            if (store && c.std) c.std[(size_t)at * LBEAMS + beam] = sd;
            if (c.loglik) {
                if (store) {
                    const float z = (pm_preprocess(c.target[(size_t)at * LBEAMS + beam]) - loc) / sd;
                    term = ((-0.5f * z) * z - pm_log(sd)) - PM_HALF_LOG_2PI;
                }
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) term = term + __shfl_xor(term, m, 64);
                if (cc == 0) part[row * LPS + p] = term;
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_decode_lidar_kernel(RcLidarDecodeCall c) {
    extern __shared__ float ld_lds[];
    float *A = ld_lds + O_LA, *B = ld_lds + O_LB, *part = ld_lds + O_LP;
    const int tid = threadIdx.x, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * PM;
    const RcLidarDecodeDev &w = c.w;

    // the rows' features [stoch | deter] into A; zeros for rows past the end
    for (int idx = tid; idx < PM * LFEAT; idx += PT) {
        const int row = idx / LFEAT, j = idx - row * LFEAT;
        const int64_t q = row0 + row;
        float v = 0.0f;
        if (q < c.n_rows) {
            if (c.features) v = c.features[(size_t)q * LFEAT + j];
            else v = c.state[(size_t)pm_car(c.rows, (int)q) * RC_POLICY_STATE + j];
        }
        A[row * LAS + j] = v;
    }
    __syncthreads();

    // dense1: tiles wave, wave + 4 of the 8; no activation; A -> B
    {
        const int col[2] = {32 * wave, 32 * wave + 128};
        pm_f32x16 acc[2];
        pm_bias<2>(acc, w.d1_b, col, cc);
        pm_gemm<2>(acc, A + cc * LAS + half, LFEAT / 2, w.d1_w + (size_t)half * RC_LDEC_H1 + cc, RC_LDEC_H1, col);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) B[pm_row(r, half) * LBS + col[t] + cc] = acc[t][r];
    }
    __syncthreads();

    // dense2: tiles wave, wave + 4, wave + 8, wave + 12 of the 16; ReLU; B -> A (the features are read no more)
    {
        const int col[4] = {32 * wave, 32 * wave + 128, 32 * wave + 256, 32 * wave + 384};
        pm_f32x16 acc[4];
        pm_bias<4>(acc, w.d2_b, col, cc);
        pm_gemm<4>(acc, B + cc * LBS + half, RC_LDEC_H1 / 2, w.d2_w + (size_t)half * RC_LDEC_H2 + cc, RC_LDEC_H2, col);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[t][r];
                A[pm_row(r, half) * LAS + col[t] + cc] = v > 0.0f ? v : 0.0f;
            }
    }
    __syncthreads();

    // params: two pairs (loc tile, scale tile) per pass, passes wave, wave + 4, ... of the 17
#pragma unroll 1
    for (int dp = wave; dp < LPAIRS / 2; dp += 4) {
        const int p0 = 2 * dp, p1 = p0 + 1;
        const int col[4] = {32 * p0, RC_LDEC_HALF + 32 * p0, 32 * p1, RC_LDEC_HALF + 32 * p1};
        pm_f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        pm_gemm<4>(acc, A + cc * LAS + half, RC_LDEC_H2 / 2, w.p_w + (size_t)half * RC_LDEC_LD + cc, RC_LDEC_LD, col);
        ld_pair(c, acc[0], acc[1], p0, row0, lane, part);
        ld_pair(c, acc[2], acc[3], p1, row0, lane, part);
    }
    if (!c.loglik) return;                                                         // (the same for every thread)
    __syncthreads();
    if (tid < PM) {
        const int64_t q = row0 + tid;
        int64_t at = -1;
        if (q < c.n_rows) at = c.features ? q : (int64_t)pm_car(c.rows, (int)q);
        float s = 0.0f;
#pragma unroll 1
        for (int p = 0; p < LPAIRS; ++p) s = s + part[tid * LPS + p];
        if (at >= 0) c.loglik[at] = s;
    }
}

hipError_t rck_decode_lidar_prepare() {
    return hipFuncSetAttribute((const void *)rc_policy_decode_lidar_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLidarLdsBytes);
}

hipError_t rck_launch_decode_lidar(const RcLidarDecodeCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.n_rows + PM - 1) / PM);
    hipExtLaunchKernelGGL(rc_policy_decode_lidar_kernel, dim3(blocks), dim3(PT), (uint32_t)kLidarLdsBytes, s, start, stop, 0u, c);
    return hipGetLastError();
}
