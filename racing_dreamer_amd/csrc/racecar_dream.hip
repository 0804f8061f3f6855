// rc_policy_dream_ahead: planning in the latent.  K candidate action sequences per start latent are carried
// H steps through the world model open loop (ros_agent/models/dreamer/models.py:44-52 `RSSM.imagine`) and scored by the reward
// head (dreamer/models.py:301-318 DenseDecoder) in one launch: the dream's counterpart of rc_look_ahead, in the binary32 arithmetic
// of item 15 (tests/policy_dream_spec.c is the CPU restatement).
//
// The workgroup geometry is rc_policy_imagine_kernel's (racecar_policy_tiles.h): four waves, 32 rows, activations in the two
// [32][417] buffers X and Y, the latent in Z [32][233] = deter 200 | stoch 30 | action 2 for the whole horizon.  A row is a pair
// (start s, candidate k), row = s K + k: a workgroup loads its rows' latents from start row / K (K = 5: seven starts in a
// workgroup; K = 33: a start's rows straddle two), reads actions_in by row, and runs per step, with one barrier after each:
//   prior  img1 Z->X, GRU (X, Z.deter)->Y, img2 Y->X (and Y->Z.deter), img3 X->Z.stoch
//   head   h0 Z->X, h1 X->Y, hout Y->reward[t] and the row's return                (skipped when only final_feature is asked for)
// The actor is never run.  The return ret = sum_t w_t r_t, w_t = discount^t, is accumulated in LDS by the lane that holds the
// head's one output column, in step order (acc = fmaf(w, r, acc); w = w * discount): no second pass over a reward array.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int ZS = 233;                        // row stride of Z (41 mod 64, odd: the 32 rows on 32 banks)
constexpr int Z_STOCH = RC_POLICY_DETER, Z_ACTION = RC_POLICY_DETER + RC_POLICY_STOCH;
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
// behind X, Y, Z per row: the output row s K + k and the state row of its start (int64, -1 past the end), the return
constexpr size_t kLdsBytes = (size_t)(2 * PM * XS + PM * ZS) * sizeof(float) + PM * (2 * sizeof(int64_t) + sizeof(float));
constexpr size_t kLdsBytesSampled = kLdsBytes + (size_t)PM * (PN + 4) * sizeof(float);      // + a step's normals and the draw's key

enum { DK_ELU = 0, DK_STOCH = 1, DK_REWARD = 2 };

struct DrLayer {
    const float *a;          // LDS input, first column; rows `as` apart
    int k;
    const float *a2;         // second part of the input (weight rows k ..), or k2 = 0
    int k2, as;
    const float *w, *b;
    int ld, n;
    float *d;                // LDS output, first column; rows `ds` apart
    int ds, kind;
};

struct DrRows {
    const int64_t *out;      // [32] s K + k of the row in the caller's arrays, -1 past the end
    float *ret;              // [32] the return so far
    const float *normals;    // [32][PN] (sampled only)
};

// One wave's tiles of a layer.  PAIR = false: the 32-column tiles at col0, col0 + 128, ...  PAIR = true (TN = 2, the sampled
// mode's img3): mean columns in tile 0, raw std columns in tile 1 of the ld-64 image.
template <int TN, bool PAIR>
__device__ __forceinline__ void dr_dense(const RcDreamCall &c, const DrLayer &L, const DrRows &R, int t, float weight, int col0, int lane) {
    const int cc = lane & 31, half = lane >> 5;
    int col[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) col[i] = col0 + (PAIR ? 32 : 128) * i;
    pm_f32x16 acc[TN];
    pm_bias<TN>(acc, L.b, col, cc);
    pm_gemm<TN>(acc, L.a + cc * L.as + half, L.k / 2, L.w + (size_t)half * L.ld + cc, L.ld, col);
    if (L.k2) pm_gemm<TN>(acc, L.a2 + cc * L.as + half, L.k2 / 2, L.w + (size_t)(L.k + half) * L.ld + cc, L.ld, col);
    if constexpr (PAIR) {
        if (cc >= L.n) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = pm_row(r, half);
            L.d[row * L.ds + cc] = fmaf(pm_softplus(acc[1][r]) + PM_STOCH_MIN_STD, R.normals[row * PN + cc], acc[0][r]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int j = col[i] + cc;
            if (j >= L.n) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = pm_row(r, half);
                const float v = acc[i][r];
                if (L.kind == DK_ELU) {
                    L.d[row * L.ds + j] = pm_elu(v);
                } else if (L.kind == DK_STOCH) {           // mode `mean`: the prior's mean is the new stoch
                    L.d[row * L.ds + j] = v;
                } else {                                   // the head's one column: this lane alone owns its 16 rows' returns
                    const int64_t q = R.out[row];
                    if (q < 0) continue;
                    if (c.reward) c.reward[(size_t)q * c.horizon + t] = v;
                    R.ret[row] = fmaf(weight, v, R.ret[row]);
                }
            }
        }
    }
}

template <bool SAMPLED>
__device__ __forceinline__ void dr_dream(const RcDreamCall &c) {
    extern __shared__ float dr_lds[];
    float *X = dr_lds, *Y = dr_lds + PM * XS, *Z = dr_lds + 2 * PM * XS;
    int64_t *out_row = (int64_t *)(Z + PM * ZS);             // [32]  (the floats before it are a multiple of 8 bytes)
    int64_t *lat_row = out_row + PM;                         // [32]
    float *ret = (float *)(lat_row + PM);                    // [32]
    uint32_t *key = (uint32_t *)(ret + PM);                  // [32][4] start id lo, hi, candidate, -   (sampled only)
    float *normals = (float *)(key + 4 * PM);                // [32][PN]                                 (sampled only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PM;
    const int H = c.horizon;

    if (tid < PM) {
        const int64_t q = row0 + tid;
        int64_t o = -1, l = -1;
        uint64_t id = 0;
        uint32_t k = 0;
        if (q < c.n_rows) {
            const int64_t s = q / c.candidates;
            k = (uint32_t)(q - s * c.candidates);
            if (c.live) {
                // start s is the car of row s of the mask's rows; its arrays are indexed by car, its draws by the global car id
                l = pm_car(c.rows, (int)s);
                id = (uint64_t)c.rows.first_env * (uint64_t)c.rows.cars_per_env + (uint64_t)l;
            } else {
                l = s;
                id = c.row_offset + (uint64_t)s;
            }
            o = l * c.candidates + k;
        }
        out_row[tid] = o;
        lat_row[tid] = l;
        ret[tid] = 0.0f;
        if constexpr (SAMPLED) {
            key[4 * tid] = (uint32_t)id;
            key[4 * tid + 1] = (uint32_t)(id >> 32);
            key[4 * tid + 2] = k;
            key[4 * tid + 3] = 0u;
        }
    }
    __syncthreads();
    // the latent of the row's start: stoch | deter of its state row (the two action columns are not read); zero rows past the end
    for (int idx = tid; idx < PM * ZS; idx += PT) {
        const int row = idx / ZS, j = idx - row * ZS;
        const int64_t l = lat_row[row];
        float v = 0.0f;
        if (l >= 0 && j < FEAT) v = c.state[(size_t)l * RC_POLICY_STATE + (j < RC_POLICY_DETER ? RC_POLICY_STOCH + j : j - RC_POLICY_DETER)];
        Z[idx] = v;
    }
    __syncthreads();

    const DrRows R{out_row, ret, normals};
    const bool head = c.ret != nullptr || c.reward != nullptr;
    float weight = 1.0f;
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        if constexpr (SAMPLED) {
            // thread (row, block) = (tid / 8, tid % 8) draws block `block` of step t of its row
            const int row = tid >> 3, blk = tid & 7;
            const uint32_t *k = key + 4 * row;
            float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (out_row[row] >= 0) pm_dream_normal_block(k[0], k[1], k[2], (uint32_t)t, (uint32_t)blk, c.seed_lo, c.seed_hi, n);
#pragma unroll
            for (int i = 0; i < 4; ++i) normals[row * PN + 4 * blk + i] = n[i];
        }
        if (tid < 2 * PM) {
            const int row = tid >> 1, j = tid & 1;
            const int64_t q = out_row[row];
            Z[row * ZS + Z_ACTION + j] = q >= 0 ? pm_clamp_action(c.actions_in[((size_t)q * H + t) * 2 + j]) : 0.0f;
        }
        __syncthreads();
        const int last = head ? 6 : 3;
#pragma unroll 1
        for (int layer = 0; layer < last; ++layer) {
            DrLayer L;
            switch (layer) {
            case 0: L = {Z + Z_STOCH, 32, nullptr, 0, ZS, c.w.img1_w, c.w.img1_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, DK_ELU}; break;
            case 1: L = {Y, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img2_w, c.wi.img2_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, DK_ELU}; break;
            case 2: L = {X, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img3_w, c.wi.img3_b, RC_POLICY_LDPAIR, RC_POLICY_STOCH, Z + Z_STOCH, ZS, DK_STOCH}; break;
            case 3: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.wi.rh_w[0], c.wi.rh_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, DK_ELU}; break;
            case 4: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rh_w[1], c.wi.rh_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, DK_ELU}; break;
            default: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rout_w, c.wi.rout_b, RC_POLICY_LDSMALL, 1, nullptr, 0, DK_REWARD}; break;
            }
            if (layer == 1) {
                // the new deter into the latent: the GRU's readers of the old one are through, nothing reads Z in this phase
                for (int idx = tid; idx < PM * RC_POLICY_DETER; idx += PT) {
                    const int row = idx / RC_POLICY_DETER, j = idx - row * RC_POLICY_DETER;
                    Z[row * ZS + j] = Y[row * XS + j];
                }
            }
            const int n_tiles = (L.n + 31) / 32;
            const int mine = wave < n_tiles ? (n_tiles - wave + 3) / 4 : 0;      // tiles wave, wave + 4, ...
            if (SAMPLED && layer == 2) {
                if (wave == 0) dr_dense<2, true>(c, L, R, t, weight, 0, lane);
            } else if (mine == 1) dr_dense<1, false>(c, L, R, t, weight, 32 * wave, lane);
            else if (mine == 2) dr_dense<2, false>(c, L, R, t, weight, 32 * wave, lane);
            else if (mine == 3) dr_dense<3, false>(c, L, R, t, weight, 32 * wave, lane);
            else if (mine == 4) dr_dense<4, false>(c, L, R, t, weight, 32 * wave, lane);
            __syncthreads();
            if (layer != 0) continue;

            // ---- GRU on x = X[0, 200) and h = Z[0, 200), as rc_policy_kernel's: the new deter goes to Y[0, 200)
#pragma unroll 1
            for (int jt = wave; jt < RC_POLICY_LD200 / 32; jt += 4) {
                const int col[3] = {32 * jt, RC_POLICY_LD200 + 32 * jt, 2 * RC_POLICY_LD200 + 32 * jt};
                pm_f32x16 mx[3], mh[3];
                pm_bias<3>(mx, c.w.gru_b, col, cc);
                pm_gemm<3>(mx, X + cc * XS + half, RC_POLICY_DETER / 2, c.w.gru_k + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
                pm_bias<3>(mh, c.w.gru_b + RC_POLICY_LDGRU, col, cc);
                pm_gemm<3>(mh, Z + cc * ZS + half, RC_POLICY_DETER / 2, c.w.gru_r + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
                const int j = 32 * jt + cc;
                if (j < RC_POLICY_DETER) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = pm_row(r, half);
                        Y[row * XS + j] = pm_gru(mx[0][r], mx[1][r], mx[2][r], mh[0][r], mh[1][r], mh[2][r], Z[row * ZS + j]);
                    }
                }
            }
            __syncthreads();
        }
        weight = weight * c.discount;
    }
    // what leaves the CU at the end: the returns, and the feature [stoch', deter'] after step H - 1 (the last layer's barrier is behind us)
    if (c.ret && tid < PM && out_row[tid] >= 0) c.ret[out_row[tid]] = ret[tid];
    if (c.final_feature) {
        for (int idx = tid; idx < PM * FEAT; idx += PT) {
            const int row = idx / FEAT, j = idx - row * FEAT;
            const int64_t q = out_row[row];
            if (q >= 0) c.final_feature[(size_t)q * FEAT + j] = Z[row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH)];
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_dream_kernel(RcDreamCall c) { dr_dream<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_dream_sampled_kernel(RcDreamCall c) { dr_dream<true>(c); }

hipError_t rck_dream_prepare() {
    const hipError_t e = hipFuncSetAttribute((const void *)rc_policy_dream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)rc_policy_dream_sampled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytesSampled);
}

hipError_t rck_launch_dream(const RcDreamCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.n_rows + PM - 1) / PM);
    if (!c.sample) hipExtLaunchKernelGGL(rc_policy_dream_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytes, s, start, stop, 0u, c);
    else hipExtLaunchKernelGGL(rc_policy_dream_sampled_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytesSampled, s, start, stop, 0u, c);
    return hipGetLastError();
}
