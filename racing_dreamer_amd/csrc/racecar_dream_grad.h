// The backward machinery of the dream: what racecar_dream_grad.hip and racecar_returns_grad.hip share
// on top of racecar_rollout.h - the per-step record of the prior's activations and its layout in a row's stash, the GRU with its gates
// kept, the transposed-product wrapper and its ladder, and the prior step's vector-Jacobian product (stoch', img3, img2, the GRU and
// img1).  Every product is a k-ascending MFMA chain from zero over a transposed weight image (RcDreamGradDev).
// Not part of the public interface.
#pragma once
#include "racecar_env.h"
#include "racecar_rollout.h"

#define RC_DREAM_GRAD_STASH 2240

namespace {

constexpr int LDT = RC_POLICY_LDT;
// per (row, t): x1 200 | z, r, c, hh 4 x 200 | h 200 | x2 200 | raw std 30 (+ 10) | the reward head's a1 400 | a2 400
enum { S_X1 = 0, S_Z = 200, S_R = 400, S_C = 600, S_HH = 800, S_H = 1000, S_X2 = 1200, S_RAW = 1400, S_A1 = 1440, S_A2 = 1840 };
static_assert(2 * RC_POLICY_DETER <= XS && RC_POLICY_LD400 <= XS, "X and Y hold two 200-unit cotangents side by side");

__device__ __forceinline__ float dg_elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }

// n columns of the 32 rows of an LDS buffer into the rows' stash at `dst` (row 0's; rows `stride` apart)
__device__ __forceinline__ void dg_keep(const float *src, int ss, int n, float *dst, size_t stride, int tid) {
    for (int idx = tid; idx < PM * n; idx += PT) {
        const int row = idx / n, j = idx - row * n;
        dst[row * stride + j] = src[row * ss + j];
    }
}

// ro_gru with the gates kept: z, r, the candidate and the recurrent candidate column hh go to the stash of step t
__device__ __forceinline__ void dg_gru(const RcPolicyDev &w, const float *X, const float *Z, float *Y, float *st, size_t stride, int wave, int lane) {
    const int cc = lane & 31, half = lane >> 5;
#pragma unroll 1
    for (int jt = wave; jt < RC_POLICY_LD200 / 32; jt += 4) {
        const int col[3] = {32 * jt, RC_POLICY_LD200 + 32 * jt, 2 * RC_POLICY_LD200 + 32 * jt};
        pm_f32x16 mx[3], mh[3];
        pm_bias<3>(mx, w.gru_b, col, cc);
        pm_gemm<3>(mx, X + cc * XS + half, RC_POLICY_DETER / 2, w.gru_k + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
        pm_bias<3>(mh, w.gru_b + RC_POLICY_LDGRU, col, cc);
        pm_gemm<3>(mh, Z + cc * ZS + half, RC_POLICY_DETER / 2, w.gru_r + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
        const int j = 32 * jt + cc;
        if (j < RC_POLICY_DETER) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = pm_row(r, half);
                // pm_gru, its gates named
                const float z = pm_sigmoid(mx[0][r] + mh[0][r]);
                const float rg = pm_sigmoid(mx[1][r] + mh[1][r]);
                const float hh = mh[2][r];
                const float cand = pm_tanh(mx[2][r] + rg * hh);
                Y[row * XS + j] = z * Z[row * ZS + j] + (1.0f - z) * cand;
                float *s = st + row * stride + j;
                s[S_Z] = z;
                s[S_R] = rg;
                s[S_C] = cand;
                s[S_HH] = hh;
            }
        }
    }
}

// One wave's 32-column tiles col0, col0 + 128, ... of a transposed product: a chain from zero, k ascending over the input's one
// or two parts (rows `as` apart); epi(row, j, v) for the columns j < n
template <int TN, class Epi>
__device__ __forceinline__ void dg_dense(const float *a, int k, const float *a2, int k2, int as, const float *w, int ld, int n, int col0, int lane,
                                         Epi &&epi) {
    const int cc = lane & 31, half = lane >> 5;
    int col[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) col[i] = col0 + 128 * i;
    pm_f32x16 acc[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    pm_gemm<TN>(acc, a + cc * as + half, k / 2, w + (size_t)half * ld + cc, ld, col);
    if (k2) pm_gemm<TN>(acc, a2 + cc * as + half, k2 / 2, w + (size_t)(k + half) * ld + cc, ld, col);
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int j = col[i] + cc;
        if (j >= n) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) epi(pm_row(r, half), j, acc[i][r]);
    }
}

// the ladder over a 400-unit image (13 tiles: 4, 3, 3, 3) and over a 256-column image (8 tiles: 2 each)
template <class Epi>
__device__ __forceinline__ void dg_layer400(const float *a, int k, const float *w, int wave, int lane, Epi &&epi) {
    if (wave == 0) dg_dense<4>(a, k, nullptr, 0, XS, w, RC_POLICY_LD400, RC_POLICY_UNITS, 0, lane, epi);
    else dg_dense<3>(a, k, nullptr, 0, XS, w, RC_POLICY_LD400, RC_POLICY_UNITS, 32 * wave, lane, epi);
}
template <class Epi>
__device__ __forceinline__ void dg_layer256(const float *a, int k, const float *a2, int k2, const float *w, int n, int wave, int lane, Epi &&epi) {
    dg_dense<2>(a, k, a2, k2, XS, w, LDT, n, 32 * wave, lane, epi);
}

// The prior step's vector-Jacobian product, steps 3-7 of item 23: Z holds g = the cotangent on the feature after step t (deter at
// [0, 200), stoch at [200, 230)) and leaves with the carry of step t - 1; `st` is step t's record in row 0's stash, `normals` the
// step's draws (sampled only).  act(row, j, v): delta in[30 + j], the cotangent on action j.  Seven barriers, the last one behind
// img1.  racecar_returns_grad.hip's; racecar_dream_grad.hip keeps the same steps written out in its loop (change both): called from
// there the compiler allocates that kernel's registers differently, and its device code is pinned byte for byte
// (profiles/policy_returns_grad_code_identity.txt).
template <bool SAMPLED, class Act>
__device__ __forceinline__ void dg_prior_back(const RcDreamGradDev &wt, float *X, float *Y, float *Z, const float *st, size_t stride,
                                              const float *normals, int tid, Act &&act) {
    const int wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    // 3. stoch': [delta mean | delta raw] -> X[0, 60)
    for (int idx = tid; idx < PM * RC_POLICY_STOCH; idx += PT) {
        const int row = idx / RC_POLICY_STOCH, j = idx - row * RC_POLICY_STOCH;
        const float gs = Z[row * ZS + Z_STOCH + j];
        X[row * XS + j] = gs;
        if constexpr (SAMPLED) X[row * XS + RC_POLICY_STOCH + j] = (gs * normals[row * PN + j]) * pm_sigmoid(st[row * stride + S_RAW + j]);
    }
    __syncthreads();
    // 4. img3: delta x2 -> Y[0, 200)
    dg_layer256(X, SAMPLED ? 2 * RC_POLICY_STOCH : RC_POLICY_STOCH, nullptr, 0, wt.img3_t, RC_POLICY_DETER, wave, lane,
                [&](int row, int j, float v) { Y[row * XS + j] = v * dg_elu_grad(st[row * stride + S_X2 + j]); });
    __syncthreads();
    // 5. img2: delta d = (delta x2 img2^T) + g_deter, in place
    dg_layer256(Y, RC_POLICY_DETER, nullptr, 0, wt.img2_t, RC_POLICY_DETER, wave, lane, [&](int row, int j, float v) {
        float *z = Z + row * ZS + j;
        *z = v + *z;
    });
    __syncthreads();
    // 6. GRU: Y = [delta z | delta r], X = [delta c | delta hh].  (A thread asks for the stash entries of U elements before it uses
    // the first: one wave per SIMD hides no latency by itself.)
    {
        constexpr int U = 5;
        static_assert(PM * RC_POLICY_DETER % (PT * U) == 0, "whole batches");
#pragma unroll 1
        for (int base = tid; base < PM * RC_POLICY_DETER; base += PT * U) {
            float kz[U], kr[U], kc[U], khh[U], kh[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = base + u * PT, row = idx / RC_POLICY_DETER, j = idx - row * RC_POLICY_DETER;
                const float *s = st + row * stride + j;
                kz[u] = s[S_Z]; kr[u] = s[S_R]; kc[u] = s[S_C]; khh[u] = s[S_HH]; kh[u] = s[S_H];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = base + u * PT, row = idx / RC_POLICY_DETER, j = idx - row * RC_POLICY_DETER;
                const float dd = Z[row * ZS + j], z = kz[u], r = kr[u], cd = kc[u], hh = khh[u], h = kh[u];
                const float dz = ((dd * (h - cd)) * z) * (1.0f - z);
                const float dc = (dd * (1.0f - z)) * (1.0f - cd * cd);
                Y[row * XS + j] = dz;
                Y[row * XS + RC_POLICY_DETER + j] = ((dc * hh) * r) * (1.0f - r);
                X[row * XS + j] = dc;
                X[row * XS + RC_POLICY_DETER + j] = dc * r;
            }
        }
    }
    __syncthreads();
    {
        // delta x1 = ([dz | dr | dc] gru_k^T) elu'(x1): held in registers until X's readers are through, then -> X[0, 200)
        const int col[2] = {32 * wave, 32 * wave + 128};
        pm_f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        pm_gemm<2>(acc, Y + cc * XS + half, RC_POLICY_DETER, wt.gruk_t + (size_t)half * LDT + cc, LDT, col);
        pm_gemm<2>(acc, X + cc * XS + half, RC_POLICY_DETER / 2, wt.gruk_t + (size_t)(2 * RC_POLICY_DETER + half) * LDT + cc, LDT, col);
        // carry_deter = fmaf(delta d, z, [dz | dr | dhh] gru_r^T), in place
        dg_layer256(Y, 2 * RC_POLICY_DETER, X + RC_POLICY_DETER, RC_POLICY_DETER, wt.grur_t, RC_POLICY_DETER, wave, lane, [&](int row, int j, float v) {
            float *z = Z + row * ZS + j;
            *z = fmaf(*z, st[row * stride + S_Z + j], v);
        });
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = col[i] + cc;
            if (j >= RC_POLICY_DETER) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = pm_row(r, half);
                X[row * XS + j] = acc[i][r] * dg_elu_grad(st[row * stride + S_X1 + j]);
            }
        }
    }
    __syncthreads();
    // 7. img1: delta in -> the carry's stoch, and the two action columns to the unit
    if (wave == 0)
        dg_dense<1>(X, RC_POLICY_DETER, nullptr, 0, XS, wt.img1_t, 32, 32, 0, lane, [&](int row, int j, float v) {
            if (j < RC_POLICY_STOCH) Z[row * ZS + Z_STOCH + j] = v;
            else act(row, j - RC_POLICY_STOCH, v);
        });
    __syncthreads();
}

}  // namespace

// W [..][src_ld] -> W^T [k_n][dst_ld] on stream `s` (rc_policy_dream_grad_transpose_kernel): row k of the image is column
// (k / group) group_ld + k % group of W, its first n entries W's rows, the padding zero
void rck_dream_grad_transpose(const float *w, int src_ld, int group, int group_ld, int k_n, int n, int dst_ld, float *t, hipStream_t s);
