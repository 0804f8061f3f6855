// rc_policy_act: one step of the reference's deployed Dreamer agent (ros_agent/models/dreamer/racing_dreamer.py:61-80 `action`;
// models.py:61-87 RSSM.obs_step / img_step, :339-364 ActionDecoder) for every car, deterministic mode (posterior mean,
// tanh(mean)), in the binary32 arithmetic of DESIGN.md §2 item 12: every dense layer is acc = bias, then acc = fmaf(x[k], W[k][j], acc)
// for k ascending - which is what the f32-input MFMA computes from its C operand.  The sampled modes (item 14: the posterior
// sampled; the best of 100 tanh-normal draws, dreamer/tools.py:301-321, or one draw plus exploration noise, models.py:189-202)
// are a second instantiation of the same body, rc_policy_sampled_kernel.
//
// One workgroup of four waves owns 32 cars = the rows of v_mfma_f32_32x32x2_f32 tiles and runs the whole network on them: the
// activations stay in two [32][417] LDS buffers (X, Y), the weights are read from L2 straight into the B operand (lane l reads
// W[2s + (l >> 5)][col + (l & 31)]: two 128-byte rows per request), the A operand from LDS (lane l: row l & 31, k = 2s + (l >> 5);
// stride 417 = 33 mod 64 keeps the 32 rows on 32 banks).  A wave takes the 32-column tiles w, w + 4, ... of a layer, all of them
// over the whole k range with one accumulator each: no split over k, no reduction across waves.  DESIGN.md §4 (rc_policy_kernel) has the
// arithmetic behind the choice (M = 32 cars per pass over the 4.4 MB of weights) and the measured cost.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int SCK = 120;                       // beams per staged piece of the scan (9 pieces)
constexpr int N_BEAMS = 1080;
constexpr size_t kLdsBytes = (size_t)2 * PM * XS * sizeof(float) + PM * sizeof(int);
// the sampled modes keep per car, behind `cars`: the PN normals (30 of the posterior, 2 unused, the 4 of block 8), the draw's key
// (global env, episode, agent step, slot) and the actor's distribution (mu 0, mu 1, sd 0, sd 1)
constexpr size_t kLdsBytesSampled = kLdsBytes + (size_t)PM * (PN + 4 + 4) * sizeof(float);

struct PmSampleLds {
    float *normals;          // [32][PN]
    uint32_t *key;           // [32][4]
    float *dist;             // [32][4]
};

// component j of a car's raw action: into the state, and into action_in as the env's convention wants it
__device__ __forceinline__ void pm_command(const RcPolicyCall &c, int car, int j, float a) {
    c.state[(size_t)car * RC_POLICY_STATE + RC_POLICY_STOCH + RC_POLICY_DETER + j] = a;
    c.actions[2 * (size_t)car + j] = c.raw_actions ? a : pm_postprocess(a, j ? c.lo1 : c.lo0, j ? c.hi1 : c.hi0);
}

enum { PK_ELU = 0, PK_STOCH = 1, PK_ACTION = 2 };

struct PmLayer {
    const float *a;          // LDS input [32][XS], first column of the layer's input
    int k;
    const float *w, *b;
    int ld, n;
    float *d;                // LDS output, first column
    int kind;
};

template <int TN>
__device__ __forceinline__ void pm_dense_tiles(const RcPolicyCall &c, const PmLayer &L, const int *cars, int wave, int lane) {
    const int cc = lane & 31, half = lane >> 5;
    int col[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) col[t] = 32 * (wave + 4 * t);
    pm_f32x16 acc[TN];
    pm_bias<TN>(acc, L.b, col, cc);
    pm_gemm<TN>(acc, L.a + cc * XS + half, L.k / 2, L.w + (size_t)half * L.ld + cc, L.ld, col);
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int j = col[t] + cc;
        if (j >= L.n) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = pm_row(r, half);
            const float v = acc[t][r];
            if (L.kind == PK_ELU) {
                L.d[row * XS + j] = pm_elu(v);
            } else if (L.kind == PK_STOCH) {          // posterior mean = the new stoch: next layer's input and the state
                L.d[row * XS + j] = v;
                const int car = cars[row];
                if (car >= 0) c.state[(size_t)car * RC_POLICY_STATE + j] = v;
            } else {                                   // the 2 mean columns of the actor's output layer
                const int car = cars[row];
                if (car < 0) continue;
                const float *hn = c.w.hnorm;
                const float act = hn ? pm_action_normalized(v, hn[j], hn[2 + j], hn[4 + j], hn[6 + j]) : pm_action_plain(v);
                pm_command(c, car, j, act);
            }
        }
    }
}

// The two layers whose std columns the sampled modes read (obs2, hout), one wave: mean columns in tile 0, std columns in tile 1
// of an ld-64 image, so acc[0][r] and acc[1][r] are mean and raw std of the same (car, column).  PK_STOCH: stoch = mean + std n
// -> the next layer's input and the state; PK_ACTION: the actor's mu and sd -> sm.dist.
__device__ __forceinline__ void pm_dense_pair(const RcPolicyCall &c, const PmLayer &L, const int *cars, const PmSampleLds &sm, int lane) {
    const int cc = lane & 31, half = lane >> 5;
    const int col[2] = {0, 32};
    pm_f32x16 acc[2];
    pm_bias<2>(acc, L.b, col, cc);
    pm_gemm<2>(acc, L.a + cc * XS + half, L.k / 2, L.w + (size_t)half * L.ld + cc, L.ld, col);
    if (cc >= L.n) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = pm_row(r, half);
        if (L.kind == PK_STOCH) {
            const float sd = pm_softplus(acc[1][r]) + PM_STOCH_MIN_STD;
            const float v = fmaf(sd, sm.normals[row * PN + cc], acc[0][r]);
            L.d[row * XS + cc] = v;
            const int car = cars[row];
            if (car >= 0) c.state[(size_t)car * RC_POLICY_STATE + cc] = v;
        } else {
            float mu, sd;
            pm_actor_dist(acc[0][r], acc[1][r], c.ws.hnorm4, cc, mu, sd);
            sm.dist[4 * row + cc] = mu;
            sm.dist[4 * row + 2 + cc] = sd;
        }
    }
}

// The action of the sampled modes from sm.dist: 8 lanes per car.  deploy: lane i of the 8 scores the candidates of blocks
// i, i + 8, ... < 50 (two per block, ascending), the 8 are reduced to the highest score, the lowest index among equals; explore:
// the one draw of block 8.  Then the exploration noise and the clip, and the command (pm_command).
__device__ __forceinline__ void pm_sampled_action(const RcPolicyCall &c, const int *cars, const PmSampleLds &sm, int tid) {
    const int row = tid >> 3, sub = tid & 7;
    const int car = cars[row];
    const uint32_t *key = sm.key + 4 * row;
    const float mu0 = sm.dist[4 * row], mu1 = sm.dist[4 * row + 1], sd0 = sm.dist[4 * row + 2], sd1 = sm.dist[4 * row + 3];
    float n0 = sm.normals[row * PN + 32], n1 = sm.normals[row * PN + 33];
    if (c.mode == RC_POLICY_MODE_DEPLOY) {
        float best = 0.0f;
        int best_i = -1;
#pragma unroll 1
        for (int b = sub; b < PM_CANDIDATES / 2; b += 8) {
            float n[4];
            pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_CANDIDATES + (uint32_t)b, c.rows.seed_lo, c.rows.seed_hi, n);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float sc = pm_score_term(n[2 * h], fmaf(sd0, n[2 * h], mu0)) + pm_score_term(n[2 * h + 1], fmaf(sd1, n[2 * h + 1], mu1));
                if (best_i < 0 || sc > best) { best = sc; best_i = 2 * b + h; }
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            const float o = __shfl_xor(best, m);
            const int oi = __shfl_xor(best_i, m);
            if (o > best || (o == best && oi < best_i)) { best = o; best_i = oi; }
        }
        if (sub == 0) {
            float n[4];
            pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_CANDIDATES + (uint32_t)(best_i >> 1), c.rows.seed_lo, c.rows.seed_hi, n);
            n0 = (best_i & 1) ? n[2] : n[0];
            n1 = (best_i & 1) ? n[3] : n[1];
        }
    }
    if (sub != 0 || car < 0) return;
    const float a[2] = {pm_explore(pm_tanh(fmaf(sd0, n0, mu0)), c.expl_amount, sm.normals[row * PN + 34]),
                        pm_explore(pm_tanh(fmaf(sd1, n1, mu1)), c.expl_amount, sm.normals[row * PN + 35])};
#pragma unroll
    for (int j = 0; j < 2; ++j) pm_command(c, car, j, a[j]);
}

template <bool SAMPLED>
__device__ __forceinline__ void pm_policy(const RcPolicyCall &c) {
    extern __shared__ float pm_lds[];
    float *X = pm_lds, *Y = pm_lds + PM * XS;
    int *cars = (int *)(pm_lds + 2 * PM * XS);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * PM;
    PmSampleLds sm{};

    if (tid < PM) cars[tid] = pm_car(c.rows, row0 + tid);
    if constexpr (SAMPLED) {
        // the car's key and its posterior normals, with block 8: the single action sample and the exploration noise
        sm.normals = (float *)(cars + PM);
        sm.key = (uint32_t *)(sm.normals + PM * PN);
        sm.dist = (float *)(sm.key + 4 * PM);
        const int row = tid >> 3, blk = tid & 7;
        const int car = pm_car(c.rows, row0 + row);
        float n[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t key[4] = {0u, 0u, 0u, 0u};
        if (car >= 0) {
            const int e = car / c.rows.cars_per_env;
            key[0] = c.rows.first_env + (uint32_t)e;
            key[1] = c.rows.episode[e];
            key[2] = (uint32_t)c.rows.agent_steps[e];
            key[3] = (uint32_t)(car - e * c.rows.cars_per_env);
            pm_normal_block(key[0], key[1], key[2], key[3], (uint32_t)blk, c.rows.seed_lo, c.rows.seed_hi, n);
            if (blk == 0) pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_ACTION, c.rows.seed_lo, c.rows.seed_hi, m);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sm.normals[row * PN + 4 * blk + i] = n[i];
            if (blk == 0) {
                sm.normals[row * PN + 32 + i] = m[i];
                sm.key[4 * row + i] = key[i];
            }
        }
    }
    // the latent of the cars: Y[0, 200) = deter, Y[200, 232) = stoch | previous raw action; zero for a car whose observation opens
    // an episode (racing_dreamer.py:66-70: state None) and for rows past the end
    pm_load_latent(c.rows, c.state, Y, XS, row0, tid, [&](int car, int) { return c.fresh[car] == 0; });
    __syncthreads();

#pragma unroll 1
    for (int layer = 0; layer < 7; ++layer) {
        PmLayer L;
        switch (layer) {
        case 0: L = {Y + RC_POLICY_DETER, 32, c.w.img1_w, c.w.img1_b, RC_POLICY_LD200, RC_POLICY_DETER, X, PK_ELU}; break;
        case 1: L = {Y, RC_POLICY_DETER, c.w.obs2_w, c.w.obs2_b, RC_POLICY_LDSMALL, RC_POLICY_STOCH, X + 170, PK_STOCH}; break;
        case 2: L = {X + 170, 230, c.w.h_w[0], c.w.h_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, Y, PK_ELU}; break;
        case 3: L = {Y, RC_POLICY_UNITS, c.w.h_w[1], c.w.h_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, X, PK_ELU}; break;
        case 4: L = {X, RC_POLICY_UNITS, c.w.h_w[2], c.w.h_b[2], RC_POLICY_LD400, RC_POLICY_UNITS, Y, PK_ELU}; break;
        case 5: L = {Y, RC_POLICY_UNITS, c.w.h_w[3], c.w.h_b[3], RC_POLICY_LD400, RC_POLICY_UNITS, X, PK_ELU}; break;
        default: L = {X, RC_POLICY_UNITS, c.w.hout_w, c.w.hout_b, RC_POLICY_LDSMALL, 2, nullptr, PK_ACTION}; break;
        }
        const int n_tiles = L.ld / 32;
        const int mine = wave < n_tiles ? (n_tiles - wave + 3) / 4 : 0;      // tiles wave, wave + 4, ...
        if (SAMPLED && (layer == 1 || layer == 6)) {
            L.w = layer == 1 ? c.ws.obs2_w : c.ws.hout_w;
            L.b = layer == 1 ? c.ws.obs2_b : c.ws.hout_b;
            L.ld = RC_POLICY_LDPAIR;
            if (wave == 0) pm_dense_pair(c, L, cars, sm, lane);
        } else if (mine == 1) pm_dense_tiles<1>(c, L, cars, wave, lane);
        else if (mine == 2) pm_dense_tiles<2>(c, L, cars, wave, lane);
        else if (mine == 3) pm_dense_tiles<3>(c, L, cars, wave, lane);
        else if (mine == 4) pm_dense_tiles<4>(c, L, cars, wave, lane);
        __syncthreads();
        if (layer != 0) continue;

        // ---- GRU on x = X[0, 200) and h = Y[0, 200): the new deter goes to X[200, 400) and to the state
#pragma unroll 1
        for (int jt = wave; jt < RC_POLICY_LD200 / 32; jt += 4) {
            const int col[3] = {32 * jt, RC_POLICY_LD200 + 32 * jt, 2 * RC_POLICY_LD200 + 32 * jt};
            pm_f32x16 mx[3], mh[3];
            pm_bias<3>(mx, c.w.gru_b, col, cc);
            pm_gemm<3>(mx, X + cc * XS + half, RC_POLICY_DETER / 2, c.w.gru_k + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
            pm_bias<3>(mh, c.w.gru_b + RC_POLICY_LDGRU, col, cc);
            pm_gemm<3>(mh, Y + cc * XS + half, RC_POLICY_DETER / 2, c.w.gru_r + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
            const int j = 32 * jt + cc;
            if (j < RC_POLICY_DETER) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = pm_row(r, half);
                    const float h = pm_gru(mx[0][r], mx[1][r], mx[2][r], mh[0][r], mh[1][r], mh[2][r], Y[row * XS + j]);
                    X[row * XS + RC_POLICY_DETER + j] = h;
                    const int car = cars[row];
                    if (car >= 0) c.state[(size_t)car * RC_POLICY_STATE + RC_POLICY_STOCH + j] = h;
                }
            }
        }
        __syncthreads();

        // ---- obs1 on [deter, embed]: deter from X[200, 400), the scan in 9 pieces of 120 beams staged through X[0, 120)
        // (clip / 15 - 0.5 applied on the way in); ELU -> Y[0, 200)
        {
            constexpr int PER = PM * SCK / PT;                       // 15 beams per thread and piece
            float pre[PER];
            auto request = [&](int piece) {
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + PT * i, row = idx / SCK, b = idx - row * SCK;
                    const int car = cars[row];
                    pre[i] = car >= 0 ? c.lidar[(size_t)car * N_BEAMS + piece * SCK + b] : 0.0f;
                }
            };
            request(0);
            const int mine1 = (RC_POLICY_LD200 / 32 - wave + 3) / 4;      // 2, 2, 2, 1
            int col[2] = {32 * wave, 32 * (wave + 4)};
            if (mine1 < 2) col[1] = col[0];                                // (second tile unused: a valid column, never stored)
            pm_f32x16 acc[2];
            pm_bias<2>(acc, c.w.obs1_b, col, cc);
            pm_gemm<2>(acc, X + RC_POLICY_DETER + cc * XS + half, RC_POLICY_DETER / 2, c.w.obs1_w + (size_t)half * RC_POLICY_LD200 + cc,
                       RC_POLICY_LD200, col);
#pragma unroll 1
            for (int piece = 0; piece < N_BEAMS / SCK; ++piece) {
                __syncthreads();                                           // the readers of the previous piece (and of x) are through
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + PT * i, row = idx / SCK, b = idx - row * SCK;
                    X[row * XS + b] = pm_preprocess(pre[i]);
                }
                __syncthreads();
                if (piece + 1 < N_BEAMS / SCK) request(piece + 1);
                pm_gemm<2>(acc, X + cc * XS + half, SCK / 2,
                           c.w.obs1_w + (size_t)(RC_POLICY_DETER + piece * SCK + half) * RC_POLICY_LD200 + cc, RC_POLICY_LD200, col);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int j = col[t] + cc;
                if (t >= mine1 || j >= RC_POLICY_DETER) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[pm_row(r, half) * XS + j] = pm_elu(acc[t][r]);
            }
        }
        __syncthreads();
    }
    if constexpr (SAMPLED) pm_sampled_action(c, cars, sm, tid);
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_kernel(RcPolicyCall c) { pm_policy<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_sampled_kernel(RcPolicyCall c) { pm_policy<true>(c); }

hipError_t rck_policy_prepare() {
    const hipError_t e = hipFuncSetAttribute((const void *)rc_policy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)rc_policy_sampled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytesSampled);
}

hipError_t rck_launch_policy(const RcPolicyCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.rows.n_active + PM - 1) / PM);
    if (c.mode == RC_POLICY_MODE_MEAN) hipExtLaunchKernelGGL(rc_policy_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytes, s, start, stop, 0u, c);
    else hipExtLaunchKernelGGL(rc_policy_sampled_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytesSampled, s, start, stop, 0u, c);
    return hipGetLastError();
}

// ---- entry points (include/racecar_hip.h): the weight packer, rc_policy_*
namespace {

// One packed matrix of the device image (racecar_policy.h): the array it comes from and the shape that must have, its padding
// (pol_pad) and where its device pointer goes.  An array with two images (obs2, hout: mean columns, and mean | std) has two rows.
template <class W>
struct PolImage {
    const char *name;
    const rc_policy_array W::*arr;
    int rows, cols;
    bool optional;
    int gates, group, take, ld;              // ld: the leading dimension PER GATE, the image's is gates x ld (a pair image: 2 x 32 =
                                             // RC_POLICY_LDPAIR); ld 0: checked only, no image of its own
    const float *&(*dst)(rc_env &);
    size_t floats() const { return (size_t)rows * gates * ld; }
};
#define POL_DST(field) [](rc_env &e) -> const float *& { return e.field; }
constexpr int LD2 = RC_POLICY_LD200, LD4 = RC_POLICY_LD400, LDSM = RC_POLICY_LDSMALL, NST = RC_POLICY_STOCH;
using PW = rc_policy_weights;
const PolImage<PW> kPolImages[] = {
    {"gru_kernel", &PW::gru_kernel, 200, 600, false, 3, 200, 200, LD2, POL_DST(pol.gru_k)},
    {"gru_recurrent", &PW::gru_recurrent, 200, 600, false, 3, 200, 200, LD2, POL_DST(pol.gru_r)},
    {"gru_bias", &PW::gru_bias, 2, 600, false, 3, 200, 200, LD2, POL_DST(pol.gru_b)},
    {"img1_w", &PW::img1_w, 32, 200, false, 1, 200, 200, LD2, POL_DST(pol.img1_w)},
    {"img1_b", &PW::img1_b, 1, 200, false, 1, 200, 200, LD2, POL_DST(pol.img1_b)},
    // rc_policy_imagine's layers (all four or rc_policy_load leaves them out); img3 mean | std, as obs2's pair image
    {"img2_w", &PW::img2_w, 200, 200, true, 1, 200, 200, LD2, POL_DST(pol_i.img2_w)},
    {"img2_b", &PW::img2_b, 1, 200, true, 1, 200, 200, LD2, POL_DST(pol_i.img2_b)},
    {"img3_w", &PW::img3_w, 200, 60, true, 2, NST, NST, 32, POL_DST(pol_i.img3_w)},
    {"img3_b", &PW::img3_b, 1, 60, true, 2, NST, NST, 32, POL_DST(pol_i.img3_b)},
    {"obs1_w", &PW::obs1_w, 1280, 200, false, 1, 200, 200, LD2, POL_DST(pol.obs1_w)},
    {"obs1_b", &PW::obs1_b, 1, 200, false, 1, 200, 200, LD2, POL_DST(pol.obs1_b)},
    {"obs2_w", &PW::obs2_w, 200, 60, false, 1, 60, NST, LDSM, POL_DST(pol.obs2_w)},          // the mean columns only
    {"obs2_b", &PW::obs2_b, 1, 60, false, 1, 60, NST, LDSM, POL_DST(pol.obs2_b)},
    // the sampled modes' images: the mean columns in tile 0, the std columns in tile 1 (pol_pad: 2 groups of 30 / 2 columns)
    {"obs2_w", &PW::obs2_w, 200, 60, false, 2, NST, NST, 32, POL_DST(pol_s.obs2_w)},
    {"obs2_b", &PW::obs2_b, 1, 60, false, 2, NST, NST, 32, POL_DST(pol_s.obs2_b)},
    {"h0_w", &PW::h0_w, 230, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_w[0])}, {"h0_b", &PW::h0_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_b[0])},
    {"h1_w", &PW::h1_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_w[1])}, {"h1_b", &PW::h1_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_b[1])},
    {"h2_w", &PW::h2_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_w[2])}, {"h2_b", &PW::h2_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_b[2])},
    {"h3_w", &PW::h3_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_w[3])}, {"h3_b", &PW::h3_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol.h_b[3])},
    {"hout_w", &PW::hout_w, 400, 4, false, 1, 4, 2, LDSM, POL_DST(pol.hout_w)}, {"hout_b", &PW::hout_b, 1, 4, false, 1, 4, 2, LDSM, POL_DST(pol.hout_b)},
    {"hout_w", &PW::hout_w, 400, 4, false, 2, 2, 2, 32, POL_DST(pol_s.hout_w)}, {"hout_b", &PW::hout_b, 1, 4, false, 2, 2, 2, 32, POL_DST(pol_s.hout_b)},
    // the batch normalisation's four: here for the shape check alone (ld 0); rc_policy_load packs their two images itself
    {"hnorm_mean", &PW::hnorm_mean, 1, 4, true, 0, 0, 0, 0, nullptr}, {"hnorm_var", &PW::hnorm_var, 1, 4, true, 0, 0, 0, 0, nullptr},
    {"hnorm_gamma", &PW::hnorm_gamma, 1, 4, true, 0, 0, 0, 0, nullptr}, {"hnorm_beta", &PW::hnorm_beta, 1, 4, true, 0, 0, 0, 0, nullptr},
};
using PH = rc_policy_heads;
const PolImage<PH> kHeadImages[] = {
    {"reward_h0_w", &PH::reward_h0_w, 230, 400, false, 1, 400, 400, LD4, POL_DST(pol_i.rh_w[0])},
    {"reward_h0_b", &PH::reward_h0_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol_i.rh_b[0])},
    {"reward_h1_w", &PH::reward_h1_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol_i.rh_w[1])},
    {"reward_h1_b", &PH::reward_h1_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol_i.rh_b[1])},
    {"reward_hout_w", &PH::reward_hout_w, 400, 1, false, 1, 1, 1, LDSM, POL_DST(pol_i.rout_w)},
    {"reward_hout_b", &PH::reward_hout_b, 1, 1, false, 1, 1, 1, LDSM, POL_DST(pol_i.rout_b)},
};
// the critic's two heads (rc_policy_load_critic): the pcont head is optional as a whole
using PC = rc_policy_critic;
const PolImage<PC> kCriticImages[] = {
    {"value_h0_w", &PC::value_h0_w, 230, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_w[0])},
    {"value_h0_b", &PC::value_h0_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_b[0])},
    {"value_h1_w", &PC::value_h1_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_w[1])},
    {"value_h1_b", &PC::value_h1_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_b[1])},
    {"value_h2_w", &PC::value_h2_w, 400, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_w[2])},
    {"value_h2_b", &PC::value_h2_b, 1, 400, false, 1, 400, 400, LD4, POL_DST(pol_c.vh_b[2])},
    {"value_hout_w", &PC::value_hout_w, 400, 1, false, 1, 1, 1, LDSM, POL_DST(pol_c.vout_w)},
    {"value_hout_b", &PC::value_hout_b, 1, 1, false, 1, 1, 1, LDSM, POL_DST(pol_c.vout_b)},
    {"pcont_h0_w", &PC::pcont_h0_w, 230, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_w[0])},
    {"pcont_h0_b", &PC::pcont_h0_b, 1, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_b[0])},
    {"pcont_h1_w", &PC::pcont_h1_w, 400, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_w[1])},
    {"pcont_h1_b", &PC::pcont_h1_b, 1, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_b[1])},
    {"pcont_h2_w", &PC::pcont_h2_w, 400, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_w[2])},
    {"pcont_h2_b", &PC::pcont_h2_b, 1, 400, true, 1, 400, 400, LD4, POL_DST(pol_c.ph_b[2])},
    {"pcont_hout_w", &PC::pcont_hout_w, 400, 1, true, 1, 1, 1, LDSM, POL_DST(pol_c.pout_w)},
    {"pcont_hout_b", &PC::pcont_hout_b, 1, 1, true, 1, 1, 1, LDSM, POL_DST(pol_c.pout_b)},
};
#undef POL_DST
const rc_policy_sampling kPolSamplingDefault = {(uint32_t)sizeof(rc_policy_sampling), RC_POLICY_MODE_MEAN, 0u, 0.0f};

// every array of the table is there (or optional) and has its shape: `fn` and `whose` word the refusal
template <class W, size_t N>
int pol_check(const PolImage<W> (&table)[N], const W &w, const char *fn, const char *whose) {
    for (const PolImage<W> &im : table) {
        const rc_policy_array &a = w.*(im.arr);
        if (!a.data) {
            if (!im.optional) return fail(RC_ERR_INVALID, "%s: %s is missing", fn, im.name);
            continue;
        }
        if (a.rows != im.rows || a.cols != im.cols)
            return fail(RC_ERR_INVALID, "%s: %s has shape [%d, %d], %s is [%d, %d]", fn, im.name, a.rows, a.cols, whose, im.rows, im.cols);
    }
    return RC_OK;
}

// The table's images behind `img` (every row has its place, given or not: the size does not depend on the checkpoint), each on a
// 64-float boundary, zero padded: [rows][cols] (first `take` columns of every one of `gates` groups of `group` columns) ->
// [rows][gates * ld].  at[i] = row i's offset in floats.
template <class W, size_t N>
void pol_pack(const PolImage<W> (&table)[N], const W &w, std::vector<float> &img, size_t (&at)[N]) {
    for (size_t i = 0; i < N; ++i) {
        at[i] = img.size();
        img.resize(img.size() + (table[i].floats() + 63) / 64 * 64, 0.0f);
        const PolImage<W> &im = table[i];
        const float *src = (w.*(im.arr)).data;
        if (!src || !im.ld) continue;
        for (int k = 0; k < im.rows; ++k)
            for (int g = 0; g < im.gates; ++g)
                for (int j = 0; j < im.take; ++j) img[at[i] + ((size_t)k * im.gates + g) * im.ld + j] = src[(size_t)k * im.cols + g * im.group + j];
    }
}

// the device pointers of the images uploaded at `mem`: null for an array that was not given
template <class W, size_t N>
void pol_point(const PolImage<W> (&table)[N], const W &w, rc_env *env, const float *mem, const size_t (&at)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (table[i].ld) table[i].dst(*env) = (w.*(table[i].arr)).data ? mem + at[i] : nullptr;
}

// pol_pack's inverse for the images at `mem` on the device: the arrays of `w` that have a data pointer receive their [rows][cols],
// the padding dropped (written despite the const).  Synchronises the stream.
template <class W, size_t N>
int pol_unpack(const PolImage<W> (&table)[N], const W &w, rc_env *env, const float *mem) {
    size_t at[N], total = 0;
    for (size_t i = 0; i < N; ++i) {                        // pol_pack's offsets: every image on a 64-float boundary
        at[i] = total;
        total += (table[i].floats() + 63) / 64 * 64;
    }
    std::vector<float> img(total);
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipMemcpyAsync(img.data(), mem, total * sizeof(float), hipMemcpyDeviceToHost, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));
    for (size_t i = 0; i < N; ++i) {
        const PolImage<W> &im = table[i];
        float *dst = const_cast<float *>((w.*(im.arr)).data);
        if (!dst) continue;
        for (int k = 0; k < im.rows; ++k)
            for (int j = 0; j < im.cols; ++j) dst[(size_t)k * im.cols + j] = img[at[i] + (size_t)k * im.ld + j];
    }
    return RC_OK;
}

// the reward head's memory and pointers go (rc_policy_load_heads(NULL), a new rc_policy_load); the prior's layers stay
int pol_drop_heads(rc_env *env) {
    int rc = dream_grad_release(env);            // (its transposed images were made from these weights)
    if (rc) return rc;
    rc = returns_grad_release(env);              // (and rc_policy_returns_grad's)
    if (rc) return rc;
    rc = fit_release_reward(env);                // (the optimizer holds pointers into the head's memory)
    if (rc) return rc;
    if (env->pol_heads_mem) {
        HIP_TRY(hipSetDevice(env->cfg.device));
        HIP_TRY(hipStreamSynchronize(env->stream));
        (void)hipFree(env->pol_heads_mem);
        env->pol_heads_mem = nullptr;
    }
    env->pol_i.rh_w[0] = env->pol_i.rh_w[1] = env->pol_i.rh_b[0] = env->pol_i.rh_b[1] = env->pol_i.rout_w = env->pol_i.rout_b = nullptr;
    return RC_OK;
}

// the decoder's memory and pointers go (rc_policy_load_decoder(NULL), a new rc_policy_load)
int pol_drop_decoder(rc_env *env) {
    if (env->pol_dec_mem) {
        HIP_TRY(hipSetDevice(env->cfg.device));
        HIP_TRY(hipStreamSynchronize(env->stream));
        (void)hipFree(env->pol_dec_mem);
        env->pol_dec_mem = nullptr;
    }
    env->pol_d = RcDecodeDev{};
    return RC_OK;
}

// the LiDAR distance decoder's memory and pointers go (rc_policy_load_lidar_decoder(NULL), a new rc_policy_load)
int pol_drop_lidar_decoder(rc_env *env) {
    if (env->pol_ldec_mem) {
        HIP_TRY(hipSetDevice(env->cfg.device));
        HIP_TRY(hipStreamSynchronize(env->stream));
        (void)hipFree(env->pol_ldec_mem);
        env->pol_ldec_mem = nullptr;
    }
    env->pol_ld = RcLidarDecodeDev{};
    return RC_OK;
}

// rc_policy_lidar_decoder's arrays in order: the shape each must have, and the row stride of its device image
struct LdecArray { const char *name; const rc_policy_array rc_policy_lidar_decoder::*arr; int rows, cols, ld; };
using PLdec = rc_policy_lidar_decoder;
const LdecArray kLdecArrays[] = {
    {"ldec_dense1_w", &PLdec::ldec_dense1_w, 230, RC_LDEC_H1, RC_LDEC_H1}, {"ldec_dense1_b", &PLdec::ldec_dense1_b, 1, RC_LDEC_H1, RC_LDEC_H1},
    {"ldec_dense2_w", &PLdec::ldec_dense2_w, RC_LDEC_H1, RC_LDEC_H2, RC_LDEC_H2}, {"ldec_dense2_b", &PLdec::ldec_dense2_b, 1, RC_LDEC_H2, RC_LDEC_H2},
    {"ldec_params_w", &PLdec::ldec_params_w, RC_LDEC_H2, 2 * RC_LDEC_BEAMS, RC_LDEC_LD}, {"ldec_params_b", &PLdec::ldec_params_b, 1, 2 * RC_LDEC_BEAMS, RC_LDEC_LD},
};

// The decoder's device image, every array on a 64-float boundary; at[i] = array i's offset in floats.  The last layer's 2160
// columns go to two padded halves, loc at [0, 1080) and scale at [RC_LDEC_HALF, RC_LDEC_HALF + 1080), the padding zero
// (racecar_decode_lidar.hip, "the partial tile")
void pol_pack_lidar_decoder(const rc_policy_lidar_decoder &d, std::vector<float> &img, size_t (&at)[6]) {
    for (size_t i = 0; i < 6; ++i) {
        const LdecArray &a = kLdecArrays[i];
        at[i] = img.size();
        img.resize(img.size() + ((size_t)a.rows * a.ld + 63) / 64 * 64, 0.0f);
        const float *src = (d.*(a.arr)).data;
        float *dst = img.data() + at[i];
        for (int k = 0; k < a.rows; ++k)
            for (int j = 0; j < a.cols; ++j) {
                const int col = a.ld == RC_LDEC_LD && j >= RC_LDEC_BEAMS ? RC_LDEC_HALF + j - RC_LDEC_BEAMS : j;
                dst[(size_t)k * a.ld + col] = src[(size_t)k * a.cols + j];
            }
    }
}

// the critic's memory and pointers go (rc_policy_load_critic(NULL), a new rc_policy_load)
int pol_drop_critic(rc_env *env) {
    int rc = fit_release(env);           // (an optimizer holds pointers into the critic's memory)
    if (rc) return rc;
    rc = returns_grad_release(env);      // (rc_policy_returns_grad's transposed images were made from these weights)
    if (rc) return rc;
    if (env->pol_critic_mem) {
        HIP_TRY(hipSetDevice(env->cfg.device));
        HIP_TRY(hipStreamSynchronize(env->stream));
        (void)hipFree(env->pol_critic_mem);
        env->pol_critic_mem = nullptr;
    }
    env->pol_c = RcCriticDev{};
    return RC_OK;
}

// rc_policy_decoder's arrays in order: the shape each must have (a kernel as [kh kw out, in])
struct DecArray { const char *name; const rc_policy_array rc_policy_decoder::*arr; int rows, cols; };
using PDec = rc_policy_decoder;
const DecArray kDecArrays[] = {
    {"dec_h1_w", &PDec::dec_h1_w, 230, 64}, {"dec_h1_b", &PDec::dec_h1_b, 1, 64}, {"dec_h2_k", &PDec::dec_h2_k, 800, 64}, {"dec_h2_b", &PDec::dec_h2_b, 1, 32},
    {"dec_h3_k", &PDec::dec_h3_k, 400, 32}, {"dec_h3_b", &PDec::dec_h3_b, 1, 16}, {"dec_h4_k", &PDec::dec_h4_k, 288, 16}, {"dec_h4_b", &PDec::dec_h4_b, 1, 8},
    {"dec_h5_k", &PDec::dec_h5_k, 36, 8}, {"dec_h5_b", &PDec::dec_h5_b, 1, 1},
};

// The decoder's device image (RcDecodeDev says which order each array takes), every array on a 64-float boundary; at[i] = array
// i's offset in floats.  A 6 x 6 kernel's element (u, v) = (py + 2 ty, px + 2 tx) goes to tap (ty, tx) of class (py, px).
void pol_pack_decoder(const rc_policy_decoder &d, std::vector<float> &img, size_t (&at)[10]) {
    for (size_t i = 0; i < 10; ++i) {
        at[i] = img.size();
        img.resize(img.size() + ((size_t)kDecArrays[i].rows * kDecArrays[i].cols + 63) / 64 * 64, 0.0f);
        const float *src = (d.*(kDecArrays[i].arr)).data;
        float *dst = img.data() + at[i];
        const int rows = kDecArrays[i].rows, cols = kDecArrays[i].cols;
        if (i == 2) {                            // h2 [(u 5 + v) 32 + o][c] -> [c][(u 5 + v) 32 + o]
            for (int j = 0; j < rows; ++j)
                for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + j] = src[(size_t)j * cols + c];
        } else if (i == 4) {                     // h3 [u][v][o 16][c 32] -> [o / 4][u][v][c][o % 4]
            for (int uv = 0; uv < 25; ++uv)
                for (int o = 0; o < 16; ++o)
                    for (int c = 0; c < 32; ++c) dst[((size_t)((o >> 2) * 25 + uv) * 32 + c) * 4 + (o & 3)] = src[((size_t)uv * 16 + o) * 32 + c];
        } else if (i == 6 || i == 8) {           // h4 [u][v][o 8][c 16] -> [ty][tx][c][py][px][o]; h5 the same with 1 output, 8 inputs
            const int no = i == 6 ? 8 : 1, nc = cols;
            for (int u = 0; u < 6; ++u)
                for (int v = 0; v < 6; ++v)
                    for (int o = 0; o < no; ++o)
                        for (int c = 0; c < nc; ++c)
                            dst[((size_t)(((u >> 1) * 3 + (v >> 1)) * nc + c) * 4 + (u & 1) * 2 + (v & 1)) * no + o] = src[((size_t)(u * 6 + v) * no + o) * nc + c];
        } else {
            std::memcpy(dst, src, (size_t)rows * cols * sizeof(float));
        }
    }
}

// the rows of a call over the cars in `slot_mask`, and the key of their draws under `seed`
int pol_rows(rc_env *env, uint32_t slot_mask, uint64_t seed, const char *fn, RcPolicyRows *r) {
    if (slot_mask == 0) return fail(RC_ERR_INVALID, "%s: the slot mask is empty", fn);
    if (slot_mask >> env->cfg.cars_per_env)
        return fail(RC_ERR_INVALID, "%s: slot mask 0x%x names slots beyond cars_per_env = %d", fn, slot_mask, env->cfg.cars_per_env);
    *r = RcPolicyRows{};
    r->cars_per_env = env->cfg.cars_per_env;
    for (int a = 0; a < env->cfg.cars_per_env; ++a)
        if ((slot_mask >> a) & 1u) r->slots |= (uint32_t)a << (8 * r->n_slots++);
    r->n_active = env->cfg.num_envs * r->n_slots;
    r->seed_lo = seed_lo(seed); r->seed_hi = seed_hi(seed);
    r->first_env = env->params.first_env;
    r->episode = env->params.st.episode;
    r->agent_steps = env->params.st.agent_steps;
    return RC_OK;
}

// one launch on the env's stream, timed as RC_K_POLICY
template <class Call>
int pol_launch(rc_env *env, hipError_t (*launch)(const Call &, hipEvent_t, hipEvent_t, hipStream_t), const Call &c) {
    KernelTimer t;
    int rc = t.begin(env, RC_K_POLICY);
    if (rc) return rc;
    hipEvent_t ea = nullptr, eb = nullptr;
    rck_take_launch_events(&ea, &eb);
    HIP_TRY(launch(c, ea, eb, env->stream));
    return t.end();
}

}  // namespace

// rc_policy_unload and rc_destroy; the caller has synchronised the stream
void policy_release(rc_env *env) {
    (void)fit_release_actor(env);        // (the optimizer holds pointers into the policy's memory)
    (void)pol_drop_heads(env);
    (void)pol_drop_decoder(env);
    (void)pol_drop_lidar_decoder(env);
    (void)pol_drop_critic(env);
    if (env->pol_mem) (void)hipFree(env->pol_mem);
    if (env->pol_state) (void)hipFree(env->pol_state);
    env->pol_mem = env->pol_state = nullptr;
    env->pol = RcPolicyDev{};
    env->pol_s = RcPolicySampleDev{};
    env->pol_i = RcImagineDev{};
}

extern "C" {

int rc_policy_load(rc_env *env, const rc_policy_weights *w) {
    if (!w) return fail(RC_ERR_INVALID, "rc_policy_weights is NULL");
    if (w->struct_size != sizeof(rc_policy_weights))
        return fail(RC_ERR_INVALID, "rc_policy_weights.struct_size %u != %zu", w->struct_size, sizeof(rc_policy_weights));
    int rc = pol_check(kPolImages, *w, "rc_policy_load", "the agent's");
    if (rc) return rc;
    const int n_norm = !!w->hnorm_mean.data + !!w->hnorm_var.data + !!w->hnorm_gamma.data + !!w->hnorm_beta.data;
    if (n_norm != 0 && n_norm != 4) return fail(RC_ERR_INVALID, "rc_policy_load: %d of the four hnorm_* arrays given (all or none)", n_norm);
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    std::vector<float> img;
    size_t at[sizeof(kPolImages) / sizeof(kPolImages[0])];
    pol_pack(kPolImages, *w, img, at);
    // the actor's batch normalisation, mean | sqrt(var + eps) | gamma | beta: of the 2 mean columns, and of all four (the sampled modes)
    const size_t o_norm = img.size(), o_norm4 = o_norm + 64;
    img.resize(o_norm4 + 64, 0.0f);
    if (n_norm) {
        const float *part[4] = {w->hnorm_mean.data, w->hnorm_var.data, w->hnorm_gamma.data, w->hnorm_beta.data};
        for (int p = 0; p < 4; ++p)
            for (int j = 0; j < 4; ++j) {
                const float v = p == 1 ? std::sqrt(part[p][j] + 1e-3f) : part[p][j];        // binary32: Keras' epsilon, IEEE square root
                img[o_norm4 + 4 * p + j] = v;
                if (j < 2) img[o_norm + 2 * p + j] = v;
            }
    }
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(rck_policy_prepare());
    HIP_TRY(rck_imagine_prepare());
    HIP_TRY(rck_dream_prepare());
    HIP_TRY(rck_dream_grad_prepare());
    HIP_TRY(rck_returns_grad_prepare());
    HIP_TRY(rck_observe_prepare());
    HIP_TRY(rck_decode_prepare());
    HIP_TRY(rck_decode_lidar_prepare());
    HIP_TRY(rck_returns_prepare());
    rc = fit_release_actor(env);                            // new weights: the moments and the transposed images are another actor's
    if (rc) return rc;
    rc = pol_drop_heads(env);
    if (rc) return rc;
    rc = pol_drop_decoder(env);
    if (rc) return rc;
    rc = pol_drop_lidar_decoder(env);
    if (rc) return rc;
    rc = pol_drop_critic(env);
    if (rc) return rc;
    if (!env->pol_mem) HIP_TRY(hipMalloc((void **)&env->pol_mem, img.size() * sizeof(float)));
    const size_t state_bytes = (size_t)env->n_cars * RC_POLICY_STATE * sizeof(float);
    if (!env->pol_state) HIP_TRY(hipMalloc((void **)&env->pol_state, state_bytes));
    HIP_TRY(hipMemcpyAsync(env->pol_mem, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipMemsetAsync(env->pol_state, 0, state_bytes, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    pol_point(kPolImages, *w, env, env->pol_mem, at);
    env->pol.hnorm = n_norm ? env->pol_mem + o_norm : nullptr;
    env->pol_s.hnorm4 = n_norm ? env->pol_mem + o_norm4 : nullptr;
    if (!env->pol_i.img2_w || !env->pol_i.img2_b || !env->pol_i.img3_w || !env->pol_i.img3_b) env->pol_i = RcImagineDev{};
    env->pol_sampling = kPolSamplingDefault;
    return RC_OK;
}

int rc_policy_unload(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    policy_release(env);
    env->pol_sampling = kPolSamplingDefault;
    return RC_OK;
}

int rc_policy_set_sampling(rc_env *env, const rc_policy_sampling *sp) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_set_sampling: no policy loaded (rc_policy_load)");
    rc_policy_sampling want = kPolSamplingDefault;
    if (sp) {
        if (sp->struct_size != sizeof(rc_policy_sampling))
            return fail(RC_ERR_INVALID, "rc_policy_sampling.struct_size %u != %zu", sp->struct_size, sizeof(rc_policy_sampling));
        if (sp->mode != RC_POLICY_MODE_MEAN && sp->mode != RC_POLICY_MODE_DEPLOY && sp->mode != RC_POLICY_MODE_EXPLORE)
            return fail(RC_ERR_INVALID, "rc_policy_set_sampling: unknown mode %d", sp->mode);
        if (!(sp->expl_amount >= 0.0f) || std::isinf(sp->expl_amount))
            return fail(RC_ERR_INVALID, "rc_policy_set_sampling: expl_amount %g is not a finite number >= 0", (double)sp->expl_amount);
        want = *sp;
    }
    env->pol_sampling = want;
    return RC_OK;
}

int rc_policy_get_sampling(rc_env *env, rc_policy_sampling *out) {
    if (!env || !out) return fail(RC_ERR_INVALID, "NULL argument");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_get_sampling: no policy loaded (rc_policy_load)");
    *out = env->pol_sampling;
    return RC_OK;
}

int rc_policy_act(rc_env *env, uint32_t slot_mask) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_act: no policy loaded (rc_policy_load)");
    if (!env->was_reset) return fail(RC_ERR_NEEDS_RESET, "Must reset environment.");
    RcPolicyCall c{};
    int rc = pol_rows(env, slot_mask, env->pol_sampling.seed, "rc_policy_act", &c.rows);
    if (rc) return rc;
    if (env->cfg.lidar_transform != RC_LIDAR_METRES) return fail(RC_ERR_INVALID, "rc_policy_act reads the scan in metres (lidar_transform RC_LIDAR_METRES)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol;
    c.lidar = env->params.out.lidar;
    c.fresh = env->params.out.fresh;
    c.state = env->pol_state;
    c.actions = env->actions_in;
    c.raw_actions = env->cfg.remap_actions != 0;
    c.mode = env->pol_sampling.mode;
    c.expl_amount = env->pol_sampling.expl_amount;
    c.ws = env->pol_s;
    c.lo0 = env->cfg.action_low[0]; c.lo1 = env->cfg.action_low[1]; c.hi0 = env->cfg.action_high[0]; c.hi1 = env->cfg.action_high[1];
    return pol_launch(env, rck_launch_policy, c);
}

int rc_policy_state(rc_env *env, void **dev_ptr, size_t *bytes) {
    if (!env || !dev_ptr || !bytes) return fail(RC_ERR_INVALID, "NULL argument");
    if (!env->pol_state) return fail(RC_ERR_INVALID, "rc_policy_state: no policy loaded (rc_policy_load)");
    *dev_ptr = env->pol_state;
    *bytes = (size_t)env->n_cars * RC_POLICY_STATE * sizeof(float);
    return RC_OK;
}

int rc_policy_load_heads(rc_env *env, const rc_policy_heads *h) {
    if (!h) {
        if (!env) return fail(RC_ERR_INVALID, "env is NULL");
        return pol_drop_heads(env);
    }
    if (h->struct_size != sizeof(rc_policy_heads))
        return fail(RC_ERR_INVALID, "rc_policy_heads.struct_size %u != %zu", h->struct_size, sizeof(rc_policy_heads));
    const int rc = pol_check(kHeadImages, *h, "rc_policy_load_heads", "the reward head's");
    if (rc) return rc;
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_heads: no policy loaded (rc_policy_load)");
    std::vector<float> img;
    size_t at[sizeof(kHeadImages) / sizeof(kHeadImages[0])];
    pol_pack(kHeadImages, *h, img, at);
    HIP_TRY(hipSetDevice(env->cfg.device));
    const int rc_grad = dream_grad_release(env);            // new weights: the transposed images are another head's
    if (rc_grad) return rc_grad;
    const int rc_rgrad = returns_grad_release(env);         // (rc_policy_returns_grad's as well)
    if (rc_rgrad) return rc_rgrad;
    const int rc_fit = fit_release_reward(env);             // and the moments another head's
    if (rc_fit) return rc_fit;
    if (!env->pol_heads_mem) HIP_TRY(hipMalloc((void **)&env->pol_heads_mem, img.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(env->pol_heads_mem, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    pol_point(kHeadImages, *h, env, env->pol_heads_mem, at);
    return RC_OK;
}

int rc_policy_imagine(rc_env *env, const rc_policy_imagine_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_imagine_args))
        return fail(RC_ERR_INVALID, "rc_policy_imagine_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_imagine_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_imagine: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_imagine: the policy was loaded without the prior's layers img2 / img3");
    if (a->horizon < 1 || a->horizon > RC_POLICY_IMAGINE_MAX_HORIZON)
        return fail(RC_ERR_INVALID, "rc_policy_imagine: horizon %d is outside [1, %d]", a->horizon, RC_POLICY_IMAGINE_MAX_HORIZON);
    if (a->mode != RC_POLICY_IMAGINE_MEAN && a->mode != RC_POLICY_IMAGINE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_imagine: unknown mode %d", a->mode);
    RcImagineCall c{};
    const int rc = pol_rows(env, a->slot_mask, a->seed, "rc_policy_imagine", &c.rows);
    if (rc) return rc;
    if (!a->reward && !a->actions && !a->features && !a->reward_start) return fail(RC_ERR_INVALID, "rc_policy_imagine: no output asked for");
    if ((a->reward || a->reward_start) && !env->pol_i.rout_w)
        return fail(RC_ERR_INVALID, "rc_policy_imagine: a reward is asked for and no reward head is loaded (rc_policy_load_heads)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol;
    c.ws = env->pol_s;
    c.wi = env->pol_i;
    c.state = env->pol_state;
    c.horizon = a->horizon;
    c.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.actions_in = a->actions_in;
    c.reward = a->reward; c.actions = a->actions; c.features = a->features; c.reward_start = a->reward_start;
    return pol_launch(env, rck_launch_imagine, c);
}

int rc_policy_dream_ahead(rc_env *env, const rc_policy_dream_ahead_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_dream_ahead_args))
        return fail(RC_ERR_INVALID, "rc_policy_dream_ahead_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_dream_ahead_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: the policy was loaded without the prior's layers img2 / img3");
    if (a->horizon < 1 || a->horizon > RC_POLICY_IMAGINE_MAX_HORIZON)
        return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: horizon %d is outside [1, %d]", a->horizon, RC_POLICY_IMAGINE_MAX_HORIZON);
    if (a->candidates < 1) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: candidates %d is below 1", a->candidates);
    if (a->mode != RC_POLICY_IMAGINE_MEAN && a->mode != RC_POLICY_IMAGINE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: unknown mode %d", a->mode);
    if (!(a->discount >= 0.0f && a->discount <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: discount %g is not a number in [0, 1]", (double)a->discount);
    if (!a->actions_in) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: actions_in is NULL");
    if (!a->ret && !a->reward && !a->final_feature) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: no output asked for");
    if ((a->ret || a->reward) && !env->pol_i.rout_w)
        return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: a reward is asked for and no reward head is loaded (rc_policy_load_heads)");
    RcDreamCall c{};
    int64_t starts;
    if (a->state_in) {
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: a slot mask (0x%x) goes with the live latents, not with a given state_in", a->slot_mask);
        if (a->starts < 1) return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: starts %lld is below 1", (long long)a->starts);
        starts = a->starts;
        c.state = a->state_in;
        c.row_offset = a->row_offset;
    } else {
        const int rc = pol_rows(env, a->slot_mask, a->seed, "rc_policy_dream_ahead", &c.rows);
        if (rc) return rc;
        starts = c.rows.n_active;
        c.state = env->pol_state;
        c.live = 1;
    }
    if (starts > (int64_t)INT32_MAX / a->candidates)
        return fail(RC_ERR_INVALID, "rc_policy_dream_ahead: %lld starts x %d candidates is not below 2^31", (long long)starts, a->candidates);
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol;
    c.wi = env->pol_i;
    c.candidates = a->candidates;
    c.n_rows = starts * a->candidates;
    c.horizon = a->horizon;
    c.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.seed_lo = seed_lo(a->seed); c.seed_hi = seed_hi(a->seed);
    c.discount = a->discount;
    c.actions_in = a->actions_in;
    c.ret = a->ret; c.reward = a->reward; c.final_feature = a->final_feature;
    return pol_launch(env, rck_launch_dream, c);
}

int rc_policy_dream_grad(rc_env *env, const rc_policy_dream_grad_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_dream_grad_args))
        return fail(RC_ERR_INVALID, "rc_policy_dream_grad_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_dream_grad_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: the policy was loaded without the prior's layers img2 / img3");
    if (!env->pol_i.rout_w) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: no reward head is loaded (rc_policy_load_heads)");
    if (a->horizon < 1 || a->horizon > RC_POLICY_IMAGINE_MAX_HORIZON)
        return fail(RC_ERR_INVALID, "rc_policy_dream_grad: horizon %d is outside [1, %d]", a->horizon, RC_POLICY_IMAGINE_MAX_HORIZON);
    if (a->candidates < 1) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: candidates %d is below 1", a->candidates);
    if (a->mode != RC_POLICY_IMAGINE_MEAN && a->mode != RC_POLICY_IMAGINE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: unknown mode %d", a->mode);
    if (!(a->discount >= 0.0f && a->discount <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_dream_grad: discount %g is not a number in [0, 1]", (double)a->discount);
    if (a->chunk_rows < 0) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: chunk_rows %lld is below 0", (long long)a->chunk_rows);
    if (!a->actions_in) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: actions_in is NULL");
    if (!a->grad_actions && !a->grad_state && !a->ret && !a->reward) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: no output asked for");
    RcDreamGradCall c{};
    int64_t starts;
    if (a->state_in) {
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: a slot mask (0x%x) goes with the live latents, not with a given state_in", a->slot_mask);
        if (a->starts < 1) return fail(RC_ERR_INVALID, "rc_policy_dream_grad: starts %lld is below 1", (long long)a->starts);
        starts = a->starts;
        c.d.state = a->state_in;
        c.d.row_offset = a->row_offset;
    } else {
        const int rc = pol_rows(env, a->slot_mask, a->seed, "rc_policy_dream_grad", &c.d.rows);
        if (rc) return rc;
        starts = c.d.rows.n_active;
        c.d.state = env->pol_state;
        c.d.live = 1;
    }
    if (starts > (int64_t)INT32_MAX / a->candidates)
        return fail(RC_ERR_INVALID, "rc_policy_dream_grad: %lld starts x %d candidates is not below 2^31", (long long)starts, a->candidates);
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.d.w = env->pol;
    c.d.wi = env->pol_i;
    c.d.candidates = a->candidates;
    c.d.n_rows = starts * a->candidates;
    c.d.horizon = a->horizon;
    c.d.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.d.seed_lo = seed_lo(a->seed); c.d.seed_hi = seed_hi(a->seed);
    c.d.discount = a->discount;
    c.d.actions_in = a->actions_in;
    c.d.ret = a->ret; c.d.reward = a->reward;
    c.grad_actions = a->grad_actions; c.grad_state = a->grad_state;
    return dream_grad_run(env, c, a->chunk_rows);
}

int rc_policy_load_critic(rc_env *env, const rc_policy_critic *h) {
    if (!h) {
        if (!env) return fail(RC_ERR_INVALID, "env is NULL");
        return pol_drop_critic(env);
    }
    if (h->struct_size != sizeof(rc_policy_critic))
        return fail(RC_ERR_INVALID, "rc_policy_critic.struct_size %u != %zu", h->struct_size, sizeof(rc_policy_critic));
    const int rc = pol_check(kCriticImages, *h, "rc_policy_load_critic", "the head's");
    if (rc) return rc;
    int n_pcont = 0;
    for (const PolImage<PC> &im : kCriticImages) n_pcont += im.optional && (h->*(im.arr)).data;
    if (n_pcont != 0 && n_pcont != 8) return fail(RC_ERR_INVALID, "rc_policy_load_critic: %d of the eight pcont_* arrays given (all or none)", n_pcont);
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_critic: no policy loaded (rc_policy_load)");
    std::vector<float> img;
    size_t at[sizeof(kCriticImages) / sizeof(kCriticImages[0])];
    pol_pack(kCriticImages, *h, img, at);
    HIP_TRY(hipSetDevice(env->cfg.device));
    const int rc_fit = fit_release(env);                    // new weights: the moments and the transposed images are another critic's
    if (rc_fit) return rc_fit;
    const int rc_rgrad = returns_grad_release(env);         // and so are rc_policy_returns_grad's
    if (rc_rgrad) return rc_rgrad;
    if (!env->pol_critic_mem) HIP_TRY(hipMalloc((void **)&env->pol_critic_mem, img.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(env->pol_critic_mem, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    pol_point(kCriticImages, *h, env, env->pol_critic_mem, at);
    return RC_OK;
}

// The inverse of rc_policy_load_critic's packing: the images as rc_policy_fit_step last left them, the padding dropped
int rc_policy_read_critic(rc_env *env, rc_policy_critic *out) {
    if (!env || !out) return fail(RC_ERR_INVALID, "NULL argument");
    if (out->struct_size != sizeof(rc_policy_critic))
        return fail(RC_ERR_INVALID, "rc_policy_critic.struct_size %u != %zu", out->struct_size, sizeof(rc_policy_critic));
    if (!env->pol_critic_mem || !env->pol_c.vout_w) return fail(RC_ERR_INVALID, "rc_policy_read_critic: no critic loaded (rc_policy_load_critic)");
    const int rc = pol_check(kCriticImages, *out, "rc_policy_read_critic", "the head's");
    if (rc) return rc;
    for (const PolImage<PC> &im : kCriticImages)
        if (im.optional && (out->*(im.arr)).data && !env->pol_c.pout_w)
            return fail(RC_ERR_INVALID, "rc_policy_read_critic: %s is asked for and no pcont head is loaded", im.name);
    return pol_unpack(kCriticImages, *out, env, env->pol_critic_mem);
}

// The inverse of rc_policy_load_heads' packing, as rc_policy_read_critic is of the critic's
int rc_policy_read_heads(rc_env *env, rc_policy_heads *out) {
    if (!env || !out) return fail(RC_ERR_INVALID, "NULL argument");
    if (out->struct_size != sizeof(rc_policy_heads))
        return fail(RC_ERR_INVALID, "rc_policy_heads.struct_size %u != %zu", out->struct_size, sizeof(rc_policy_heads));
    if (!env->pol_heads_mem || !env->pol_i.rout_w) return fail(RC_ERR_INVALID, "rc_policy_read_heads: no reward head is loaded (rc_policy_load_heads)");
    const int rc = pol_check(kHeadImages, *out, "rc_policy_read_heads", "the reward head's");
    if (rc) return rc;
    return pol_unpack(kHeadImages, *out, env, env->pol_heads_mem);
}

// The actor's arrays inside rc_policy_load's image: rc_policy_actor's ten as an rc_policy_weights that holds them alone, so that
// kPolImages' rows - the hidden layers' images, hout's mean image and its pair image - serve the actor's own entry points
static rc_policy_weights pol_actor_as_weights(const rc_policy_actor &a) {
    rc_policy_weights w{};
    w.struct_size = (uint32_t)sizeof(rc_policy_weights);
    w.h0_w = a.h0_w; w.h0_b = a.h0_b; w.h1_w = a.h1_w; w.h1_b = a.h1_b; w.h2_w = a.h2_w; w.h2_b = a.h2_b; w.h3_w = a.h3_w; w.h3_b = a.h3_b;
    w.hout_w = a.hout_w; w.hout_b = a.hout_b;
    return w;
}

// every one of the ten is there and has the checkpoint's shape
static int pol_actor_check(const rc_policy_weights &w, const char *fn) {
    for (const PolImage<PW> &im : kPolImages) {
        if (std::strncmp(im.name, "h", 1) != 0 || !std::strncmp(im.name, "hnorm", 5)) continue;
        const rc_policy_array &a = w.*(im.arr);
        if (!a.data) return fail(RC_ERR_INVALID, "%s: %s is missing", fn, im.name);
        if (a.rows != im.rows || a.cols != im.cols)
            return fail(RC_ERR_INVALID, "%s: %s has shape [%d, %d], the actor's is [%d, %d]", fn, im.name, a.rows, a.cols, im.rows, im.cols);
    }
    return RC_OK;
}

// The inverse of rc_policy_load's packing for the actor's ten arrays, as rc_policy_fit's apply last left them: the hidden layers
// from their images, hout's four columns from the pair image (the mean image holds two of them)
int rc_policy_read_actor(rc_env *env, rc_policy_actor *out) {
    if (!env || !out) return fail(RC_ERR_INVALID, "NULL argument");
    if (out->struct_size != sizeof(rc_policy_actor))
        return fail(RC_ERR_INVALID, "rc_policy_actor.struct_size %u != %zu", out->struct_size, sizeof(rc_policy_actor));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_read_actor: no policy loaded (rc_policy_load)");
    const rc_policy_weights w = pol_actor_as_weights(*out);
    const int rc = pol_actor_check(w, "rc_policy_read_actor");
    if (rc) return rc;
    constexpr size_t N = sizeof(kPolImages) / sizeof(kPolImages[0]);
    size_t at[N], total = 0;
    for (size_t i = 0; i < N; ++i) {                        // pol_pack's offsets: every image on a 64-float boundary
        at[i] = total;
        total += (kPolImages[i].floats() + 63) / 64 * 64;
    }
    std::vector<float> img(total);
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipMemcpyAsync(img.data(), env->pol_mem, total * sizeof(float), hipMemcpyDeviceToHost, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));
    for (size_t i = 0; i < N; ++i) {
        const PolImage<PW> &im = kPolImages[i];
        float *dst = const_cast<float *>((w.*(im.arr)).data);
        if (!dst || !im.ld || (im.gates == 1 && im.take < im.cols)) continue;          // (not the actor's; hout's mean image)
        for (int k = 0; k < im.rows; ++k)
            for (int g = 0; g < im.gates; ++g)
                for (int j = 0; j < im.take; ++j) dst[(size_t)k * im.cols + g * im.group + j] = img[at[i] + ((size_t)k * im.gates + g) * im.ld + j];
    }
    return RC_OK;
}

int rc_policy_load_actor(rc_env *env, const rc_policy_actor *actor) {
    if (!env || !actor) return fail(RC_ERR_INVALID, "NULL argument");
    if (actor->struct_size != sizeof(rc_policy_actor))
        return fail(RC_ERR_INVALID, "rc_policy_actor.struct_size %u != %zu", actor->struct_size, sizeof(rc_policy_actor));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_actor: no policy loaded (rc_policy_load)");
    const rc_policy_weights w = pol_actor_as_weights(*actor);
    int rc = pol_actor_check(w, "rc_policy_load_actor");
    if (rc) return rc;
    rc = fit_release_actor(env);                            // new weights: the moments and the transposed images are another actor's
    if (rc) return rc;
    constexpr size_t N = sizeof(kPolImages) / sizeof(kPolImages[0]);
    std::vector<float> img;
    size_t at[N];
    pol_pack(kPolImages, w, img, at);                       // (the images of the arrays that are not given stay zero and are not copied)
    HIP_TRY(hipSetDevice(env->cfg.device));
    for (size_t i = 0; i < N; ++i) {
        const PolImage<PW> &im = kPolImages[i];
        if (!(w.*(im.arr)).data || !im.ld) continue;
        HIP_TRY(hipMemcpyAsync(env->pol_mem + at[i], img.data() + at[i], im.floats() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    }
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    return RC_OK;
}

int rc_policy_returns(rc_env *env, const rc_policy_returns_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_returns_args))
        return fail(RC_ERR_INVALID, "rc_policy_returns_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_returns_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_returns: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_returns: the policy was loaded without the prior's layers img2 / img3");
    const bool steps = a->reward || a->value || a->pcont || a->returns || a->weight || a->actions || a->features;
    if (!steps && !a->reward_start && !a->value_start && !a->pcont_start) return fail(RC_ERR_INVALID, "rc_policy_returns: no output asked for");
    if ((a->value || a->returns || a->value_start) && !env->pol_c.vout_w)
        return fail(RC_ERR_INVALID, "rc_policy_returns: a value is asked for and no value head is loaded (rc_policy_load_critic)");
    if ((a->reward || a->returns || a->reward_start) && !env->pol_i.rout_w)
        return fail(RC_ERR_INVALID, "rc_policy_returns: a reward is asked for and no reward head is loaded (rc_policy_load_heads)");
    if (a->pcont_start && !env->pol_c.pout_w)
        return fail(RC_ERR_INVALID, "rc_policy_returns: pcont_start is asked for and no pcont head is loaded (rc_policy_load_critic)");
    const int h_min = (a->returns || a->weight) ? 2 : (steps ? 1 : 0);
    if (a->horizon < h_min || a->horizon > RC_POLICY_IMAGINE_MAX_HORIZON)
        return fail(RC_ERR_INVALID, "rc_policy_returns: horizon %d is outside [%d, %d] (0: the *_start outputs alone; returns and weight: 2 and more)",
                    a->horizon, h_min, RC_POLICY_IMAGINE_MAX_HORIZON);
    if (a->mode != RC_POLICY_IMAGINE_MEAN && a->mode != RC_POLICY_IMAGINE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_returns: unknown mode %d", a->mode);
    if (!(a->lambda_ >= 0.0f && a->lambda_ <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_returns: lambda_ %g is not a number in [0, 1]", (double)a->lambda_);
    if (!(a->discount >= 0.0f && a->discount <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_returns: discount %g is not a number in [0, 1]", (double)a->discount);
    RcReturnsCall c{};
    if (a->state_in) {
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_returns: a slot mask (0x%x) goes with the live latents, not with a given state_in", a->slot_mask);
        if (a->starts < 1 || a->starts > (int64_t)INT32_MAX)
            return fail(RC_ERR_INVALID, "rc_policy_returns: starts %lld is outside [1, 2^31)", (long long)a->starts);
        c.n_rows = a->starts;
        c.state = a->state_in;
        c.row_offset = a->row_offset;
    } else {
        const int rc = pol_rows(env, a->slot_mask, a->seed, "rc_policy_returns", &c.rows);
        if (rc) return rc;
        c.n_rows = c.rows.n_active;
        c.state = env->pol_state;
        c.live = 1;
    }
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol;
    c.ws = env->pol_s;
    c.wi = env->pol_i;
    c.wc = env->pol_c;
    c.horizon = a->horizon;
    c.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.seed_lo = seed_lo(a->seed); c.seed_hi = seed_hi(a->seed);
    c.lambda = a->lambda_; c.discount = a->discount;
    c.actions_in = a->horizon > 0 ? a->actions_in : nullptr;
    c.reward = a->reward; c.value = a->value; c.pcont = a->pcont; c.returns = a->returns; c.weight = a->weight;
    c.actions = a->actions; c.features = a->features;
    c.reward_start = a->reward_start; c.value_start = a->value_start; c.pcont_start = a->pcont_start;
    return pol_launch(env, rck_launch_returns, c);
}

int rc_policy_returns_grad(rc_env *env, const rc_policy_returns_grad_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_returns_grad_args))
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_returns_grad_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: the policy was loaded without the prior's layers img2 / img3");
    if (!env->pol_i.rout_w) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: no reward head is loaded (rc_policy_load_heads)");
    if (!env->pol_c.vout_w) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: no value head is loaded (rc_policy_load_critic)");
    if (a->pcont_start && !env->pol_c.pout_w)
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad: pcont_start is asked for and no pcont head is loaded (rc_policy_load_critic)");
    if (a->horizon < 2 || a->horizon > RC_POLICY_IMAGINE_MAX_HORIZON)
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad: horizon %d is outside [2, %d]", a->horizon, RC_POLICY_IMAGINE_MAX_HORIZON);
    if (a->mode != RC_POLICY_IMAGINE_MEAN && a->mode != RC_POLICY_IMAGINE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: unknown mode %d", a->mode);
    if (!(a->lambda_ >= 0.0f && a->lambda_ <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad: lambda_ %g is not a number in [0, 1]", (double)a->lambda_);
    if (!(a->discount >= 0.0f && a->discount <= 1.0f))
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad: discount %g is not a number in [0, 1]", (double)a->discount);
    if (!std::isfinite(a->scale)) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: scale %g is not finite", (double)a->scale);
    if (a->chunk_rows < 0) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: chunk_rows %lld is below 0", (long long)a->chunk_rows);
    if (!a->grad_actions && !a->grad_state) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: no gradient output asked for (grad_actions, grad_state)");
    if (a->eps && a->mode != RC_POLICY_IMAGINE_SAMPLE)
        return fail(RC_ERR_INVALID, "rc_policy_returns_grad: eps is asked for in mode MEAN, which draws no action");
    if (a->eps && a->actions_in) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: eps is asked for under actions_in (open loop), which draws no action");
    RcReturnsGradCall c{};
    if (a->state_in) {
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: a slot mask (0x%x) goes with the live latents, not with a given state_in", a->slot_mask);
        if (a->starts < 1 || a->starts > (int64_t)INT32_MAX)
            return fail(RC_ERR_INVALID, "rc_policy_returns_grad: starts %lld is outside [1, 2^31)", (long long)a->starts);
        c.r.n_rows = a->starts;
        c.r.state = a->state_in;
        c.r.row_offset = a->row_offset;
    } else {
        if (a->starts) return fail(RC_ERR_INVALID, "rc_policy_returns_grad: starts %lld is given and state_in is NULL", (long long)a->starts);
        const int rc = pol_rows(env, a->slot_mask, a->seed, "rc_policy_returns_grad", &c.r.rows);
        if (rc) return rc;
        c.r.n_rows = c.r.rows.n_active;
        c.r.state = env->pol_state;
        c.r.live = 1;
    }
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.r.w = env->pol;
    c.r.ws = env->pol_s;
    c.r.wi = env->pol_i;
    c.r.wc = env->pol_c;
    c.r.horizon = a->horizon;
    c.r.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.r.seed_lo = seed_lo(a->seed); c.r.seed_hi = seed_hi(a->seed);
    c.r.lambda = a->lambda_; c.r.discount = a->discount;
    c.r.actions_in = a->actions_in;
    c.r.reward = a->reward; c.r.value = a->value; c.r.pcont = a->pcont; c.r.returns = a->returns; c.r.weight = a->weight;
    c.r.actions = a->actions; c.r.features = a->features;
    c.r.reward_start = a->reward_start; c.r.value_start = a->value_start; c.r.pcont_start = a->pcont_start;
    c.scale = a->scale;
    c.grad_actions = a->grad_actions; c.actor_features = a->actor_features; c.eps = a->eps; c.grad_state = a->grad_state;
    return returns_grad_run(env, c, a->chunk_rows);
}

int rc_policy_observe(rc_env *env, const rc_policy_observe_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_observe_args))
        return fail(RC_ERR_INVALID, "rc_policy_observe_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_observe_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_observe: no policy loaded (rc_policy_load)");
    if (!env->pol_i.img3_w) return fail(RC_ERR_INVALID, "rc_policy_observe: the policy was loaded without the prior's layers img2 / img3");
    if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_observe: rows %lld is outside [1, 2^31)", (long long)a->rows);
    if (a->length < 1 || a->length > RC_POLICY_OBSERVE_MAX_LENGTH)
        return fail(RC_ERR_INVALID, "rc_policy_observe: length %d is outside [1, %d]", a->length, RC_POLICY_OBSERVE_MAX_LENGTH);
    if (a->context < 1 || a->context > a->length)
        return fail(RC_ERR_INVALID, "rc_policy_observe: context %d is outside [1, length = %d]", a->context, a->length);
    if (a->mode != RC_POLICY_OBSERVE_MEAN && a->mode != RC_POLICY_OBSERVE_SAMPLE) return fail(RC_ERR_INVALID, "rc_policy_observe: unknown mode %d", a->mode);
    if (!a->scan || !a->actions) return fail(RC_ERR_INVALID, "rc_policy_observe: %s is NULL", !a->scan ? "scan" : "actions");
    if (!a->features && !a->post_mean && !a->post_std && !a->prior_mean && !a->prior_std && !a->kl && !a->reward && !a->state_out)
        return fail(RC_ERR_INVALID, "rc_policy_observe: no output asked for");
    if (a->reward && !env->pol_i.rout_w)
        return fail(RC_ERR_INVALID, "rc_policy_observe: a reward is asked for and no reward head is loaded (rc_policy_load_heads)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcObserveCall c{};
    c.w = env->pol;
    c.ws = env->pol_s;
    c.wi = env->pol_i;
    c.rows = a->rows;
    c.row_offset = a->row_offset;
    c.length = a->length; c.context = a->context;
    c.sample = a->mode == RC_POLICY_OBSERVE_SAMPLE;
    c.seed_lo = seed_lo(a->seed); c.seed_hi = seed_hi(a->seed);
    c.scan = a->scan; c.actions = a->actions; c.state_in = a->state_in;
    c.features = a->features; c.post_mean = a->post_mean; c.post_std = a->post_std; c.prior_mean = a->prior_mean; c.prior_std = a->prior_std;
    c.kl = a->kl; c.reward = a->reward; c.state_out = a->state_out;
    return pol_launch(env, rck_launch_observe, c);
}

int rc_policy_load_decoder(rc_env *env, const rc_policy_decoder *d) {
    if (!d) {
        if (!env) return fail(RC_ERR_INVALID, "env is NULL");
        return pol_drop_decoder(env);
    }
    if (d->struct_size != sizeof(rc_policy_decoder))
        return fail(RC_ERR_INVALID, "rc_policy_decoder.struct_size %u != %zu", d->struct_size, sizeof(rc_policy_decoder));
    for (const DecArray &a : kDecArrays) {
        const rc_policy_array &g = d->*(a.arr);
        if (!g.data) return fail(RC_ERR_INVALID, "rc_policy_load_decoder: %s is missing", a.name);
        if (g.rows != a.rows || g.cols != a.cols)
            return fail(RC_ERR_INVALID, "rc_policy_load_decoder: %s has shape [%d, %d], the decoder's is [%d, %d]", a.name, g.rows, g.cols, a.rows, a.cols);
    }
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_decoder: no policy loaded (rc_policy_load)");
    std::vector<float> img;
    size_t at[10];
    pol_pack_decoder(*d, img, at);
    HIP_TRY(hipSetDevice(env->cfg.device));
    if (!env->pol_dec_mem) HIP_TRY(hipMalloc((void **)&env->pol_dec_mem, img.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(env->pol_dec_mem, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    const float *m = env->pol_dec_mem;
    env->pol_d = RcDecodeDev{m + at[0], m + at[1], m + at[2], m + at[3], m + at[4], m + at[5], m + at[6], m + at[7], m + at[8], m + at[9]};
    return RC_OK;
}

int rc_policy_decode(rc_env *env, const rc_policy_decode_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_decode_args))
        return fail(RC_ERR_INVALID, "rc_policy_decode_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_decode_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_decode: no policy loaded (rc_policy_load)");
    if (!env->pol_d.h1_w) return fail(RC_ERR_INVALID, "rc_policy_decode: no decoder loaded (rc_policy_load_decoder)");
    if (!a->logits && !a->image && !a->mismatch) return fail(RC_ERR_INVALID, "rc_policy_decode: no output asked for");
    RcDecodeCall c{};
    if (a->features) {
        if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_decode: rows %lld is outside [1, 2^31)", (long long)a->rows);
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_decode: a slot mask (0x%x) goes with the live latents, not with given features", a->slot_mask);
        if (a->mismatch) return fail(RC_ERR_INVALID, "rc_policy_decode: mismatch compares with the cars' own RC_F_OCCUPANCY: live latents only, not given features");
        c.n_rows = a->rows;
    } else {
        const int rc = pol_rows(env, a->slot_mask, 0, "rc_policy_decode", &c.rows);
        if (rc) return rc;
        if (a->mismatch && env->cfg.obs_type == RC_OBS_LIDAR)
            return fail(RC_ERR_INVALID, "rc_policy_decode: mismatch needs the rendered RC_F_OCCUPANCY (obs_type lidar_occupancy or lidar_occupancy_reference)");
        c.n_rows = c.rows.n_active;
    }
    if (((uintptr_t)a->logits & 7u) || ((uintptr_t)a->image & 1u))
        return fail(RC_ERR_INVALID, "rc_policy_decode: logits must lie on an 8-byte boundary, image on a 2-byte boundary");
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol_d;
    c.features = a->features;
    c.state = env->pol_state;
    c.logits = a->logits; c.image = a->image; c.mismatch = a->mismatch;
    c.occupancy = env->params.out.patch;
    return pol_launch(env, rck_launch_decode, c);
}

int rc_policy_decode_loglik(rc_env *env, const rc_policy_decode_loglik_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_decode_loglik_args))
        return fail(RC_ERR_INVALID, "rc_policy_decode_loglik_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_decode_loglik_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: no policy loaded (rc_policy_load)");
    if (!env->pol_d.h1_w) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: no decoder loaded (rc_policy_load_decoder)");
    if (!a->loglik && !a->logits && !a->image) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: no output asked for");
    RcDecodeLoglikCall c{};
    if (a->features) {
        if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: rows %lld is outside [1, 2^31)", (long long)a->rows);
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: a slot mask (0x%x) goes with the live latents, not with given features", a->slot_mask);
        if (a->loglik && !a->target) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: loglik of given features needs a target image");
        c.d.n_rows = a->rows;
        c.target = a->target;
    } else {
        const int rc = pol_rows(env, a->slot_mask, 0, "rc_policy_decode_loglik", &c.d.rows);
        if (rc) return rc;
        if (a->target) return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: the live latents are scored against the cars' own RC_F_OCCUPANCY: target must be NULL");
        if (a->loglik && env->cfg.obs_type == RC_OBS_LIDAR)
            return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: loglik needs the rendered RC_F_OCCUPANCY (obs_type lidar_occupancy or lidar_occupancy_reference)");
        c.d.n_rows = c.d.rows.n_active;
        c.target = env->params.out.patch;
    }
    if (((uintptr_t)a->logits & 7u) || ((uintptr_t)a->image & 1u) || ((uintptr_t)c.target & 1u))
        return fail(RC_ERR_INVALID, "rc_policy_decode_loglik: logits must lie on an 8-byte boundary, image and target on a 2-byte boundary");
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.d.w = env->pol_d;
    c.d.features = a->features;
    c.d.state = env->pol_state;
    c.d.logits = a->logits; c.d.image = a->image;
    c.loglik = a->loglik;
    return pol_launch(env, rck_launch_decode_loglik, c);
}

int rc_policy_load_lidar_decoder(rc_env *env, const rc_policy_lidar_decoder *d) {
    if (!d) {
        if (!env) return fail(RC_ERR_INVALID, "env is NULL");
        return pol_drop_lidar_decoder(env);
    }
    if (d->struct_size != sizeof(rc_policy_lidar_decoder))
        return fail(RC_ERR_INVALID, "rc_policy_lidar_decoder.struct_size %u != %zu", d->struct_size, sizeof(rc_policy_lidar_decoder));
    for (const LdecArray &a : kLdecArrays) {
        const rc_policy_array &g = d->*(a.arr);
        if (!g.data) return fail(RC_ERR_INVALID, "rc_policy_load_lidar_decoder: %s is missing", a.name);
        if (g.rows != a.rows || g.cols != a.cols)
            return fail(RC_ERR_INVALID, "rc_policy_load_lidar_decoder: %s has shape [%d, %d], the decoder's is [%d, %d]", a.name, g.rows, g.cols, a.rows, a.cols);
    }
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_lidar_decoder: no policy loaded (rc_policy_load)");
    std::vector<float> img;
    size_t at[6];
    pol_pack_lidar_decoder(*d, img, at);
    HIP_TRY(hipSetDevice(env->cfg.device));
    if (!env->pol_ldec_mem) HIP_TRY(hipMalloc((void **)&env->pol_ldec_mem, img.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(env->pol_ldec_mem, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    const float *m = env->pol_ldec_mem;
    env->pol_ld = RcLidarDecodeDev{m + at[0], m + at[1], m + at[2], m + at[3], m + at[4], m + at[5]};
    return RC_OK;
}

int rc_policy_decode_lidar(rc_env *env, const rc_policy_decode_lidar_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_decode_lidar_args))
        return fail(RC_ERR_INVALID, "rc_policy_decode_lidar_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_decode_lidar_args));
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: no policy loaded (rc_policy_load)");
    if (!env->pol_ld.d1_w) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: no LiDAR decoder loaded (rc_policy_load_lidar_decoder)");
    if (!a->mean && !a->std && !a->loglik) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: no output asked for");
    RcLidarDecodeCall c{};
    if (a->features) {
        if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: rows %lld is outside [1, 2^31)", (long long)a->rows);
        if (a->slot_mask) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: a slot mask (0x%x) goes with the live latents, not with given features", a->slot_mask);
        if (a->loglik && !a->target) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: loglik of given features needs a target scan");
        c.n_rows = a->rows;
        c.target = a->target;
    } else {
        const int rc = pol_rows(env, a->slot_mask, 0, "rc_policy_decode_lidar", &c.rows);
        if (rc) return rc;
        if (a->target) return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: the live latents are scored against the cars' own RC_F_LIDAR: target must be NULL");
        if (a->loglik && env->cfg.lidar_transform != RC_LIDAR_METRES)
            return fail(RC_ERR_INVALID, "rc_policy_decode_lidar: loglik reads the scan in metres (lidar_transform RC_LIDAR_METRES)");
        c.n_rows = c.rows.n_active;
        c.target = env->params.out.lidar;
    }
    HIP_TRY(hipSetDevice(env->cfg.device));
    c.w = env->pol_ld;
    c.features = a->features;
    c.state = env->pol_state;
    c.mean = a->mean; c.std = a->std; c.loglik = a->loglik;
    return pol_launch(env, rck_launch_decode_lidar, c);
}

}  // extern "C"
