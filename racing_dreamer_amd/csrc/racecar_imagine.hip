// rc_policy_imagine: the reference's imagination rollouts (dreamer/models.py:213-224 `_imagine_ahead`, closed loop under the
// actor; ros_agent/models/dreamer/models.py:44-52 `RSSM.imagine`, open loop under given actions) and its reward head
// (models.py:301-318 DenseDecoder) from every car's stored latent, H steps in one launch, in the binary32 arithmetic of DESIGN.md
// §2 item 15 (tests/policy_imagine_spec.c is the CPU restatement).
//
// The workgroup geometry is rc_policy_kernel's (racecar_policy_tiles.h): four waves, 32 cars, activations in the two [32][417]
// buffers X and Y.  The latent lives in a third region Z [32][233] = deter 200 | stoch 30 | action 2 for the whole horizon: every
// layer that reads it (img1, the GRU's recurrent half, the actor's and the head's first layer) takes its A operand from there,
// the layers that write it (actor output, img3) write it in place, and the new deter goes through Y because the GRU's other
// waves still read the old one.  A 230-deep first layer is two pm_gemm calls into one accumulator: stoch's 30 rows, then
// deter's 200 - k ascending as the agent's.  Per imagined step, with one barrier after each:
//   actor  h0 Z->X, h1 X->Y, h2 Y->X, h3 X->Y, hout Y->Z.action          (skipped when the caller gives the actions)
//   prior  img1 Z->X, GRU (X, Z.deter)->Y, img2 Y->X (and Y->Z.deter), img3 X->Z.stoch
//   head   h0 Z->X, h1 X->Y, hout Y->reward[t]                            (skipped when no reward is asked for)
// Only the requested outputs leave the CU.  DESIGN.md §4 has the LDS budget and why the two first layers stay two passes.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int ZS = 233;                        // row stride of Z (41 mod 64, odd: the 32 rows on 32 banks)
constexpr int Z_STOCH = RC_POLICY_DETER, Z_ACTION = RC_POLICY_DETER + RC_POLICY_STOCH;
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
constexpr size_t kLdsBytes = (size_t)(2 * PM * XS + PM * ZS) * sizeof(float) + PM * sizeof(int);
constexpr size_t kLdsBytesSampled = kLdsBytes + (size_t)PM * (PN + 4) * sizeof(float);      // + a step's normals and the draw's key

enum { IK_ELU = 0, IK_STOCH = 1, IK_ACTION = 2, IK_REWARD = 3 };

struct ImLayer {
    const float *a;          // LDS input, first column; rows `as` apart
    int k;
    const float *a2;         // second part of the input (weight rows k ..), or k2 = 0
    int k2, as;
    const float *w, *b;
    int ld, n;
    float *d;                // LDS output, first column; rows `ds` apart
    int ds, kind;
};

// One wave's tiles of a layer.  PAIR = false: the 32-column tiles at col0, col0 + 128, ...  PAIR = true (TN = 2, the sampled
// mode's img3 and hout): mean columns in tile 0, raw std columns in tile 1 of an ld-64 image, as pm_dense_pair reads them.
template <int TN, bool PAIR>
__device__ __forceinline__ void im_dense(const RcImagineCall &c, const ImLayer &L, const int *cars, const float *normals, int t, int col0, int lane) {
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
            float v;
            if (L.kind == IK_STOCH) {
                v = fmaf(pm_softplus(acc[1][r]) + PM_STOCH_MIN_STD, normals[row * PN + cc], acc[0][r]);
            } else {
                float mu, sd;
                pm_actor_dist(acc[0][r], acc[1][r], c.ws.hnorm4, cc, mu, sd);
                v = pm_tanh(fmaf(sd, normals[row * PN + 32 + cc], mu));
                const int car = cars[row];
                if (car >= 0 && c.actions) c.actions[((size_t)car * c.horizon + t) * 2 + cc] = v;
            }
            L.d[row * L.ds + cc] = v;
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
                if (L.kind == IK_ELU) {
                    L.d[row * L.ds + j] = pm_elu(v);
                } else if (L.kind == IK_STOCH) {           // mode `mean`: the prior's mean is the new stoch
                    L.d[row * L.ds + j] = v;
                } else if (L.kind == IK_ACTION) {          // mode `mean`: tanh of the actor's mean
                    const float *hn = c.w.hnorm;
                    const float act = hn ? pm_action_normalized(v, hn[j], hn[2 + j], hn[4 + j], hn[6 + j]) : pm_action_plain(v);
                    L.d[row * L.ds + j] = act;
                    const int car = cars[row];
                    if (car >= 0 && c.actions) c.actions[((size_t)car * c.horizon + t) * 2 + j] = act;
                } else {                                   // the head's one column: t < 0 is the starting feature
                    const int car = cars[row];
                    if (car < 0) continue;
                    if (t < 0) c.reward_start[car] = v;
                    else c.reward[(size_t)car * c.horizon + t] = v;
                }
            }
        }
    }
}

template <bool SAMPLED>
__device__ __forceinline__ void im_imagine(const RcImagineCall &c) {
    extern __shared__ float im_lds[];
    float *X = im_lds, *Y = im_lds + PM * XS, *Z = im_lds + 2 * PM * XS;
    int *cars = (int *)(Z + PM * ZS);
    float *normals = (float *)(cars + PM);                   // [32][PN]   (sampled only)
    uint32_t *key = (uint32_t *)(normals + PM * PN);         // [32][4]    global env, episode, agent step, slot
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * PM;

    if (tid < PM) {
        const int car = pm_car(c.rows, row0 + tid);
        cars[tid] = car;
        if constexpr (SAMPLED) {
            uint32_t k[4] = {0u, 0u, 0u, 0u};
            if (car >= 0) {
                const int e = car / c.rows.cars_per_env;
                k[0] = c.rows.first_env + (uint32_t)e;
                k[1] = c.rows.episode[e];
                k[2] = (uint32_t)c.rows.agent_steps[e];
                k[3] = (uint32_t)(car - e * c.rows.cars_per_env);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) key[4 * tid + i] = k[i];
        }
    }
    // the latent as rc_policy_act left it (`fresh` is not looked at, the previous action not read); zero rows past the end
    pm_load_latent(c.rows, c.state, Z, ZS, row0, tid, [](int, int j) { return j < FEAT; });
    __syncthreads();

    const bool open_loop = c.actions_in != nullptr, head = c.reward != nullptr;
#pragma unroll 1
    for (int t = c.reward_start ? -1 : 0; t < c.horizon; ++t) {
        if (t >= 0) {
            if constexpr (SAMPLED) {
                // thread (row, block) = (tid / 8, tid % 8) draws block `block` of step t, the thread of block 0 also block 8
                const int row = tid >> 3, blk = tid & 7;
                const uint32_t *k = key + 4 * row;
                float n[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (cars[row] >= 0) {
                    pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, (uint32_t)blk, c.rows.seed_lo, c.rows.seed_hi, n);
                    if (blk == 0 && !open_loop) pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, PM_BLOCK_ACTION, c.rows.seed_lo, c.rows.seed_hi, m);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    normals[row * PN + 4 * blk + i] = n[i];
                    if (blk == 0) normals[row * PN + 32 + i] = m[i];
                }
            }
            if (open_loop && tid < 2 * PM) {
                const int row = tid >> 1, j = tid & 1, car = cars[row];
                const float a = car >= 0 ? pm_clamp_action(c.actions_in[((size_t)car * c.horizon + t) * 2 + j]) : 0.0f;
                Z[row * ZS + Z_ACTION + j] = a;
                if (car >= 0 && c.actions) c.actions[((size_t)car * c.horizon + t) * 2 + j] = a;
            }
            __syncthreads();
        }
        const int first = t < 0 ? 8 : (open_loop ? 5 : 0), last = (t < 0 || head) ? 11 : 8;
#pragma unroll 1
        for (int layer = first; layer < last; ++layer) {
            ImLayer L;
            switch (layer) {
            case 0: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.w.h_w[0], c.w.h_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, IK_ELU}; break;
            case 1: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[1], c.w.h_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, IK_ELU}; break;
            case 2: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[2], c.w.h_b[2], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, IK_ELU}; break;
            case 3: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[3], c.w.h_b[3], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, IK_ELU}; break;
            case 4: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, SAMPLED ? c.ws.hout_w : c.w.hout_w, SAMPLED ? c.ws.hout_b : c.w.hout_b,
                         SAMPLED ? RC_POLICY_LDPAIR : RC_POLICY_LDSMALL, 2, Z + Z_ACTION, ZS, IK_ACTION}; break;
            case 5: L = {Z + Z_STOCH, 32, nullptr, 0, ZS, c.w.img1_w, c.w.img1_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, IK_ELU}; break;
            case 6: L = {Y, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img2_w, c.wi.img2_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, IK_ELU}; break;
            case 7: L = {X, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img3_w, c.wi.img3_b, RC_POLICY_LDPAIR, RC_POLICY_STOCH, Z + Z_STOCH, ZS, IK_STOCH}; break;
            case 8: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.wi.rh_w[0], c.wi.rh_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, IK_ELU}; break;
            case 9: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rh_w[1], c.wi.rh_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, IK_ELU}; break;
            default: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rout_w, c.wi.rout_b, RC_POLICY_LDSMALL, 1, nullptr, 0, IK_REWARD}; break;
            }
            if (layer == 6) {
                // the new deter into the latent: the GRU's readers of the old one are through, nothing reads Z in this phase
                for (int idx = tid; idx < PM * RC_POLICY_DETER; idx += PT) {
                    const int row = idx / RC_POLICY_DETER, j = idx - row * RC_POLICY_DETER;
                    Z[row * ZS + j] = Y[row * XS + j];
                }
            }
            const int n_tiles = (L.n + 31) / 32;
            const int mine = wave < n_tiles ? (n_tiles - wave + 3) / 4 : 0;      // tiles wave, wave + 4, ...
            if (SAMPLED && (layer == 4 || layer == 7)) {
                if (wave == 0) im_dense<2, true>(c, L, cars, normals, t, 0, lane);
            } else if (mine == 1) im_dense<1, false>(c, L, cars, normals, t, 32 * wave, lane);
            else if (mine == 2) im_dense<2, false>(c, L, cars, normals, t, 32 * wave, lane);
            else if (mine == 3) im_dense<3, false>(c, L, cars, normals, t, 32 * wave, lane);
            else if (mine == 4) im_dense<4, false>(c, L, cars, normals, t, 32 * wave, lane);
            __syncthreads();
            if (layer != 5) continue;

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
        // feature[t] = [stoch', deter'] from the latent (its next writer is a barrier away)
        if (t >= 0 && c.features) {
            for (int idx = tid; idx < PM * FEAT; idx += PT) {
                const int row = idx / FEAT, j = idx - row * FEAT, car = cars[row];
                if (car >= 0) c.features[((size_t)car * c.horizon + t) * FEAT + j] = Z[row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH)];
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_imagine_kernel(RcImagineCall c) { im_imagine<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_imagine_sampled_kernel(RcImagineCall c) { im_imagine<true>(c); }

hipError_t rck_imagine_prepare() {
    const hipError_t e = hipFuncSetAttribute((const void *)rc_policy_imagine_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)rc_policy_imagine_sampled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytesSampled);
}

hipError_t rck_launch_imagine(const RcImagineCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.rows.n_active + PM - 1) / PM);
    if (!c.sample) hipExtLaunchKernelGGL(rc_policy_imagine_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytes, s, start, stop, 0u, c);
    else hipExtLaunchKernelGGL(rc_policy_imagine_sampled_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytesSampled, s, start, stop, 0u, c);
    return hipGetLastError();
}
