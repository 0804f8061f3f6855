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
// the sampled modes keep per car, behind `cars`: 36 normals (30 of the posterior, 2 unused, the 4 of block 8), the draw's key
// (global env, episode, agent step, slot) and the actor's distribution (mu 0, mu 1, sd 0, sd 1)
constexpr int NS = 36;
constexpr size_t kLdsBytesSampled = kLdsBytes + (size_t)PM * (NS + 4 + 4) * sizeof(float);

// row q of the call -> car index (the mask's slots of env q / n_slots), -1 past the end
__device__ __forceinline__ int pm_car(const RcPolicyCall &c, int q) {
    if (q >= c.n_active) return -1;
    const int e = q / c.n_slots, k = q - e * c.n_slots;
    return e * c.cars_per_env + (int)((c.slots >> (8 * k)) & 0xffu);
}

enum { PK_ELU = 0, PK_STOCH = 1, PK_ACTION = 2 };

struct PmSampleLds {
    float *normals;          // [32][NS]
    uint32_t *key;           // [32][4]
    float *dist;             // [32][4]
};

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
                c.state[(size_t)car * RC_POLICY_STATE + RC_POLICY_STOCH + RC_POLICY_DETER + j] = act;
                c.actions[2 * (size_t)car + j] = c.raw_actions ? act : pm_postprocess(act, j ? c.lo1 : c.lo0, j ? c.hi1 : c.hi0);
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
            const float v = fmaf(sd, sm.normals[row * NS + cc], acc[0][r]);
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
// the one draw of block 8.  Then the exploration noise and the clip, and the command as PK_ACTION writes it.
__device__ __forceinline__ void pm_sampled_action(const RcPolicyCall &c, const int *cars, const PmSampleLds &sm, int tid) {
    const int row = tid >> 3, sub = tid & 7;
    const int car = cars[row];
    const uint32_t *key = sm.key + 4 * row;
    const float mu0 = sm.dist[4 * row], mu1 = sm.dist[4 * row + 1], sd0 = sm.dist[4 * row + 2], sd1 = sm.dist[4 * row + 3];
    float n0 = sm.normals[row * NS + 32], n1 = sm.normals[row * NS + 33];
    if (c.mode == RC_POLICY_MODE_DEPLOY) {
        float best = 0.0f;
        int best_i = -1;
#pragma unroll 1
        for (int b = sub; b < PM_CANDIDATES / 2; b += 8) {
            float n[4];
            pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_CANDIDATES + (uint32_t)b, c.seed_lo, c.seed_hi, n);
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
            pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_CANDIDATES + (uint32_t)(best_i >> 1), c.seed_lo, c.seed_hi, n);
            n0 = (best_i & 1) ? n[2] : n[0];
            n1 = (best_i & 1) ? n[3] : n[1];
        }
    }
    if (sub != 0 || car < 0) return;
    const float a[2] = {pm_explore(pm_tanh(fmaf(sd0, n0, mu0)), c.expl_amount, sm.normals[row * NS + 34]),
                        pm_explore(pm_tanh(fmaf(sd1, n1, mu1)), c.expl_amount, sm.normals[row * NS + 35])};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        c.state[(size_t)car * RC_POLICY_STATE + RC_POLICY_STOCH + RC_POLICY_DETER + j] = a[j];
        c.actions[2 * (size_t)car + j] = c.raw_actions ? a[j] : pm_postprocess(a[j], j ? c.lo1 : c.lo0, j ? c.hi1 : c.hi0);
    }
}

template <bool SAMPLED>
__device__ __forceinline__ void pm_policy(const RcPolicyCall &c) {
    extern __shared__ float pm_lds[];
    float *X = pm_lds, *Y = pm_lds + PM * XS;
    int *cars = (int *)(pm_lds + 2 * PM * XS);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * PM;
    PmSampleLds sm{};

    if (tid < PM) cars[tid] = pm_car(c, row0 + tid);
    if constexpr (SAMPLED) {
        // the car's key and its posterior normals: thread (row, block) = (tid / 8, tid % 8) draws block `block`, the thread of
        // block 0 also block 8 (the single action sample and the exploration noise)
        sm.normals = (float *)(cars + PM);
        sm.key = (uint32_t *)(sm.normals + PM * NS);
        sm.dist = (float *)(sm.key + 4 * PM);
        const int row = tid >> 3, blk = tid & 7;
        const int car = pm_car(c, row0 + row);
        float n[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t key[4] = {0u, 0u, 0u, 0u};
        if (car >= 0) {
            const int e = car / c.cars_per_env;
            key[0] = c.first_env + (uint32_t)e;
            key[1] = c.episode[e];
            key[2] = (uint32_t)c.agent_steps[e];
            key[3] = (uint32_t)(car - e * c.cars_per_env);
            pm_normal_block(key[0], key[1], key[2], key[3], (uint32_t)blk, c.seed_lo, c.seed_hi, n);
            if (blk == 0) pm_normal_block(key[0], key[1], key[2], key[3], PM_BLOCK_ACTION, c.seed_lo, c.seed_hi, m);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sm.normals[row * NS + 4 * blk + i] = n[i];
            if (blk == 0) {
                sm.normals[row * NS + 32 + i] = m[i];
                sm.key[4 * row + i] = key[i];
            }
        }
    }
    // the latent of the cars: Y[0, 200) = deter, Y[200, 232) = stoch | previous raw action; zero for a car whose observation opens
    // an episode (racing_dreamer.py:66-70: state None) and for rows past the end
    for (int idx = tid; idx < PM * RC_POLICY_STATE; idx += PT) {
        const int row = idx / RC_POLICY_STATE, j = idx - row * RC_POLICY_STATE;
        const int car = pm_car(c, row0 + row);
        float v = 0.0f;
        if (car >= 0 && c.fresh[car] == 0) v = c.state[(size_t)car * RC_POLICY_STATE + j];
        int dst;
        if (j < RC_POLICY_STOCH) dst = RC_POLICY_DETER + j;
        else if (j < RC_POLICY_STOCH + RC_POLICY_DETER) dst = j - RC_POLICY_STOCH;
        else dst = j;                                               // (the action's 2 columns follow stoch's 30)
        Y[row * XS + dst] = v;
    }
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
    const unsigned blocks = (unsigned)((c.n_active + PM - 1) / PM);
    if (c.mode == RC_POLICY_MODE_MEAN) hipExtLaunchKernelGGL(rc_policy_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytes, s, start, stop, 0u, c);
    else hipExtLaunchKernelGGL(rc_policy_sampled_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytesSampled, s, start, stop, 0u, c);
    return hipGetLastError();
}

// ---- entry points (include/racecar_hip.h): the weight packer, rc_policy_*
extern "C" {

namespace {
struct PolShape { const char *name; const rc_policy_array rc_policy_weights::*arr; int rows, cols; bool used, optional; };
const PolShape kPolShapes[] = {
    {"gru_kernel", &rc_policy_weights::gru_kernel, 200, 600, true, false}, {"gru_recurrent", &rc_policy_weights::gru_recurrent, 200, 600, true, false},
    {"gru_bias", &rc_policy_weights::gru_bias, 2, 600, true, false},
    {"img1_w", &rc_policy_weights::img1_w, 32, 200, true, false}, {"img1_b", &rc_policy_weights::img1_b, 1, 200, true, false},
    {"img2_w", &rc_policy_weights::img2_w, 200, 200, false, true}, {"img2_b", &rc_policy_weights::img2_b, 1, 200, false, true},
    {"img3_w", &rc_policy_weights::img3_w, 200, 60, false, true}, {"img3_b", &rc_policy_weights::img3_b, 1, 60, false, true},
    {"obs1_w", &rc_policy_weights::obs1_w, 1280, 200, true, false}, {"obs1_b", &rc_policy_weights::obs1_b, 1, 200, true, false},
    {"obs2_w", &rc_policy_weights::obs2_w, 200, 60, true, false}, {"obs2_b", &rc_policy_weights::obs2_b, 1, 60, true, false},
    {"h0_w", &rc_policy_weights::h0_w, 230, 400, true, false}, {"h0_b", &rc_policy_weights::h0_b, 1, 400, true, false},
    {"h1_w", &rc_policy_weights::h1_w, 400, 400, true, false}, {"h1_b", &rc_policy_weights::h1_b, 1, 400, true, false},
    {"h2_w", &rc_policy_weights::h2_w, 400, 400, true, false}, {"h2_b", &rc_policy_weights::h2_b, 1, 400, true, false},
    {"h3_w", &rc_policy_weights::h3_w, 400, 400, true, false}, {"h3_b", &rc_policy_weights::h3_b, 1, 400, true, false},
    {"hout_w", &rc_policy_weights::hout_w, 400, 4, true, false}, {"hout_b", &rc_policy_weights::hout_b, 1, 4, true, false},
    {"hnorm_mean", &rc_policy_weights::hnorm_mean, 1, 4, true, true}, {"hnorm_var", &rc_policy_weights::hnorm_var, 1, 4, true, true},
    {"hnorm_gamma", &rc_policy_weights::hnorm_gamma, 1, 4, true, true}, {"hnorm_beta", &rc_policy_weights::hnorm_beta, 1, 4, true, true},
};

// [rows][n_src] (first `take` columns of every one of `gates` groups of `group` columns) -> [rows][gates * ld], zero padded
void pol_pad(std::vector<float> &dst, size_t at, const float *src, int rows, int n_src, int gates, int group, int take, int ld) {
    for (int k = 0; k < rows; ++k)
        for (int g = 0; g < gates; ++g)
            for (int j = 0; j < take; ++j) dst[at + (size_t)k * gates * ld + (size_t)g * ld + j] = src[(size_t)k * n_src + g * group + j];
}

// the reward head's memory and pointers go (rc_policy_load_heads(NULL), a new rc_policy_load); the prior's layers stay
int pol_drop_heads(rc_env *env) {
    if (env->pol_heads_mem) {
        HIP_TRY(hipSetDevice(env->cfg.device));
        HIP_TRY(hipStreamSynchronize(env->stream));
        (void)hipFree(env->pol_heads_mem);
        env->pol_heads_mem = nullptr;
    }
    env->pol_i.rh_w[0] = env->pol_i.rh_w[1] = env->pol_i.rh_b[0] = env->pol_i.rh_b[1] = env->pol_i.rout_w = env->pol_i.rout_b = nullptr;
    return RC_OK;
}

struct HeadShape { const char *name; const rc_policy_array rc_policy_heads::*arr; int rows, cols; };
const HeadShape kHeadShapes[] = {
    {"reward_h0_w", &rc_policy_heads::reward_h0_w, 230, 400}, {"reward_h0_b", &rc_policy_heads::reward_h0_b, 1, 400},
    {"reward_h1_w", &rc_policy_heads::reward_h1_w, 400, 400}, {"reward_h1_b", &rc_policy_heads::reward_h1_b, 1, 400},
    {"reward_hout_w", &rc_policy_heads::reward_hout_w, 400, 1}, {"reward_hout_b", &rc_policy_heads::reward_hout_b, 1, 1},
};
}  // namespace
}  // extern "C"

// rc_policy_unload and rc_destroy; the caller has synchronised the stream
void policy_release(rc_env *env) {
    (void)pol_drop_heads(env);
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
    int n_norm = 0;
    for (const PolShape &sh : kPolShapes) {
        const rc_policy_array &a = w->*(sh.arr);
        if (!a.data) {
            if (!sh.optional) return fail(RC_ERR_INVALID, "rc_policy_load: %s is missing", sh.name);
            continue;
        }
        if (a.rows != sh.rows || a.cols != sh.cols)
            return fail(RC_ERR_INVALID, "rc_policy_load: %s has shape [%d, %d], the agent's is [%d, %d]", sh.name, a.rows, a.cols, sh.rows, sh.cols);
        n_norm += sh.name[1] == 'n';                      // hnorm_*
    }
    if (n_norm != 0 && n_norm != 4) return fail(RC_ERR_INVALID, "rc_policy_load: %d of the four hnorm_* arrays given (all or none)", n_norm);
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    // the padded device image (racecar_policy.h): offsets in floats
    const size_t LD2 = RC_POLICY_LD200, LD4 = RC_POLICY_LD400, LDG = RC_POLICY_LDGRU, LDS = RC_POLICY_LDSMALL, LDP = RC_POLICY_LDPAIR;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
    const size_t o_img1 = take(32 * LD2), o_img1b = take(LD2), o_gk = take(200 * LDG), o_gr = take(200 * LDG), o_gb = take(2 * LDG),
                 o_obs1 = take(1280 * LD2), o_obs1b = take(LD2), o_obs2 = take(200 * LDS), o_obs2b = take(LDS),
                 o_h0 = take(230 * LD4), o_h1 = take(400 * LD4), o_h2 = take(400 * LD4), o_h3 = take(400 * LD4),
                 o_hb = take(4 * LD4), o_hout = take(400 * LDS), o_houtb = take(LDS), o_norm = take(8),
                 o_obs2s = take(200 * LDP), o_obs2sb = take(LDP), o_houts = take(400 * LDP), o_houtsb = take(LDP), o_norm4 = take(16),
                 o_img2 = take(200 * LD2), o_img2b = take(LD2), o_img3 = take(200 * LDP), o_img3b = take(LDP);
    const bool prior = w->img2_w.data && w->img2_b.data && w->img3_w.data && w->img3_b.data;      // rc_policy_imagine's layers
    std::vector<float> img(at, 0.0f);
    pol_pad(img, o_img1, w->img1_w.data, 32, 200, 1, 200, 200, (int)LD2);
    pol_pad(img, o_img1b, w->img1_b.data, 1, 200, 1, 200, 200, (int)LD2);
    pol_pad(img, o_gk, w->gru_kernel.data, 200, 600, 3, 200, 200, (int)LD2);
    pol_pad(img, o_gr, w->gru_recurrent.data, 200, 600, 3, 200, 200, (int)LD2);
    pol_pad(img, o_gb, w->gru_bias.data, 2, 600, 3, 200, 200, (int)LD2);
    pol_pad(img, o_obs1, w->obs1_w.data, 1280, 200, 1, 200, 200, (int)LD2);
    pol_pad(img, o_obs1b, w->obs1_b.data, 1, 200, 1, 200, 200, (int)LD2);
    pol_pad(img, o_obs2, w->obs2_w.data, 200, 60, 1, 60, RC_POLICY_STOCH, (int)LDS);          // the mean columns only
    pol_pad(img, o_obs2b, w->obs2_b.data, 1, 60, 1, 60, RC_POLICY_STOCH, (int)LDS);
    const rc_policy_array *hw[4] = {&w->h0_w, &w->h1_w, &w->h2_w, &w->h3_w}, *hb[4] = {&w->h0_b, &w->h1_b, &w->h2_b, &w->h3_b};
    const size_t o_h[4] = {o_h0, o_h1, o_h2, o_h3};
    for (int i = 0; i < 4; ++i) {
        pol_pad(img, o_h[i], hw[i]->data, hw[i]->rows, 400, 1, 400, 400, (int)LD4);
        pol_pad(img, o_hb + i * LD4, hb[i]->data, 1, 400, 1, 400, 400, (int)LD4);
    }
    pol_pad(img, o_hout, w->hout_w.data, 400, 4, 1, 4, 2, (int)LDS);
    pol_pad(img, o_houtb, w->hout_b.data, 1, 4, 1, 4, 2, (int)LDS);
    // the sampled modes' images: the mean columns in tile 0, the std columns in tile 1 (pol_pad: 2 groups of 30 / 2 columns)
    pol_pad(img, o_obs2s, w->obs2_w.data, 200, 60, 2, RC_POLICY_STOCH, RC_POLICY_STOCH, 32);
    pol_pad(img, o_obs2sb, w->obs2_b.data, 1, 60, 2, RC_POLICY_STOCH, RC_POLICY_STOCH, 32);
    pol_pad(img, o_houts, w->hout_w.data, 400, 4, 2, 2, 2, 32);
    pol_pad(img, o_houtsb, w->hout_b.data, 1, 4, 2, 2, 2, 32);
    if (prior) {
        pol_pad(img, o_img2, w->img2_w.data, 200, 200, 1, 200, 200, (int)LD2);
        pol_pad(img, o_img2b, w->img2_b.data, 1, 200, 1, 200, 200, (int)LD2);
        pol_pad(img, o_img3, w->img3_w.data, 200, 60, 2, RC_POLICY_STOCH, RC_POLICY_STOCH, 32);      // mean | std, as obs2's
        pol_pad(img, o_img3b, w->img3_b.data, 1, 60, 2, RC_POLICY_STOCH, RC_POLICY_STOCH, 32);
    }
    if (n_norm) {
        for (int j = 0; j < 4; ++j) {
            img[o_norm4 + j] = w->hnorm_mean.data[j];
            img[o_norm4 + 4 + j] = std::sqrt(w->hnorm_var.data[j] + 1e-3f);
            img[o_norm4 + 8 + j] = w->hnorm_gamma.data[j];
            img[o_norm4 + 12 + j] = w->hnorm_beta.data[j];
        }
        for (int j = 0; j < 2; ++j) {
            img[o_norm + j] = w->hnorm_mean.data[j];
            img[o_norm + 2 + j] = std::sqrt(w->hnorm_var.data[j] + 1e-3f);        // binary32: Keras' epsilon, IEEE square root
            img[o_norm + 4 + j] = w->hnorm_gamma.data[j];
            img[o_norm + 6 + j] = w->hnorm_beta.data[j];
        }
    }
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(rck_policy_prepare());
    HIP_TRY(rck_imagine_prepare());
    int rc = pol_drop_heads(env);
    if (rc) return rc;
    if (!env->pol_mem) HIP_TRY(hipMalloc((void **)&env->pol_mem, at * sizeof(float)));
    const size_t state_bytes = (size_t)env->n_cars * RC_POLICY_STATE * sizeof(float);
    if (!env->pol_state) HIP_TRY(hipMalloc((void **)&env->pol_state, state_bytes));
    HIP_TRY(hipMemcpyAsync(env->pol_mem, img.data(), at * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipMemsetAsync(env->pol_state, 0, state_bytes, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    const float *m = env->pol_mem;
    RcPolicyDev &d = env->pol;
    d.img1_w = m + o_img1; d.img1_b = m + o_img1b; d.gru_k = m + o_gk; d.gru_r = m + o_gr; d.gru_b = m + o_gb;
    d.obs1_w = m + o_obs1; d.obs1_b = m + o_obs1b; d.obs2_w = m + o_obs2; d.obs2_b = m + o_obs2b;
    for (int i = 0; i < 4; ++i) { d.h_w[i] = m + o_h[i]; d.h_b[i] = m + o_hb + i * LD4; }
    d.hout_w = m + o_hout; d.hout_b = m + o_houtb;
    d.hnorm = n_norm ? m + o_norm : nullptr;
    env->pol_s = RcPolicySampleDev{m + o_obs2s, m + o_obs2sb, m + o_houts, m + o_houtsb, n_norm ? m + o_norm4 : nullptr};
    env->pol_i = RcImagineDev{};
    if (prior) { env->pol_i.img2_w = m + o_img2; env->pol_i.img2_b = m + o_img2b; env->pol_i.img3_w = m + o_img3; env->pol_i.img3_b = m + o_img3b; }
    env->pol_sampling = rc_policy_sampling{(uint32_t)sizeof(rc_policy_sampling), RC_POLICY_MODE_MEAN, 0u, 0.0f};
    return RC_OK;
}

int rc_policy_unload(rc_env *env) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    policy_release(env);
    env->pol_sampling = rc_policy_sampling{(uint32_t)sizeof(rc_policy_sampling), RC_POLICY_MODE_MEAN, 0u, 0.0f};
    return RC_OK;
}

int rc_policy_set_sampling(rc_env *env, const rc_policy_sampling *sp) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_set_sampling: no policy loaded (rc_policy_load)");
    rc_policy_sampling want{(uint32_t)sizeof(rc_policy_sampling), RC_POLICY_MODE_MEAN, 0u, 0.0f};
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
    if (slot_mask == 0) return fail(RC_ERR_INVALID, "rc_policy_act: the slot mask is empty");
    if (slot_mask >> env->cfg.cars_per_env) return fail(RC_ERR_INVALID, "rc_policy_act: slot mask 0x%x names slots beyond cars_per_env = %d", slot_mask, env->cfg.cars_per_env);
    if (env->cfg.lidar_transform != RC_LIDAR_METRES) return fail(RC_ERR_INVALID, "rc_policy_act reads the scan in metres (lidar_transform RC_LIDAR_METRES)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcPolicyCall c{};
    c.w = env->pol;
    c.lidar = env->params.out.lidar;
    c.fresh = env->params.out.fresh;
    c.state = env->pol_state;
    c.actions = env->actions_in;
    c.cars_per_env = env->cfg.cars_per_env;
    for (int a = 0; a < env->cfg.cars_per_env; ++a)
        if ((slot_mask >> a) & 1u) c.slots |= (uint32_t)a << (8 * c.n_slots++);
    c.n_active = env->cfg.num_envs * c.n_slots;
    c.raw_actions = env->cfg.remap_actions != 0;
    c.mode = env->pol_sampling.mode;
    c.expl_amount = env->pol_sampling.expl_amount;
    c.seed_lo = seed_lo(env->pol_sampling.seed); c.seed_hi = seed_hi(env->pol_sampling.seed);
    c.first_env = env->params.first_env;
    c.episode = env->params.st.episode;
    c.agent_steps = env->params.st.agent_steps;
    c.ws = env->pol_s;
    c.lo0 = env->cfg.action_low[0]; c.lo1 = env->cfg.action_low[1]; c.hi0 = env->cfg.action_high[0]; c.hi1 = env->cfg.action_high[1];
    KernelTimer t;
    int rc = t.begin(env, RC_K_POLICY);
    if (rc) return rc;
    hipEvent_t ea = nullptr, eb = nullptr;
    rck_take_launch_events(&ea, &eb);
    HIP_TRY(rck_launch_policy(c, ea, eb, env->stream));
    return t.end();
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
    for (const HeadShape &sh : kHeadShapes) {
        const rc_policy_array &a = h->*(sh.arr);
        if (!a.data) return fail(RC_ERR_INVALID, "rc_policy_load_heads: %s is missing", sh.name);
        if (a.rows != sh.rows || a.cols != sh.cols)
            return fail(RC_ERR_INVALID, "rc_policy_load_heads: %s has shape [%d, %d], the reward head's is [%d, %d]", sh.name, a.rows, a.cols, sh.rows, sh.cols);
    }
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!env->pol_mem) return fail(RC_ERR_INVALID, "rc_policy_load_heads: no policy loaded (rc_policy_load)");
    const size_t LD4 = RC_POLICY_LD400, LDS = RC_POLICY_LDSMALL;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
    const size_t o_h0 = take(230 * LD4), o_h1 = take(400 * LD4), o_hb = take(2 * LD4), o_out = take(400 * LDS), o_outb = take(LDS);
    std::vector<float> img(at, 0.0f);
    pol_pad(img, o_h0, h->reward_h0_w.data, 230, 400, 1, 400, 400, (int)LD4);
    pol_pad(img, o_h1, h->reward_h1_w.data, 400, 400, 1, 400, 400, (int)LD4);
    pol_pad(img, o_hb, h->reward_h0_b.data, 1, 400, 1, 400, 400, (int)LD4);
    pol_pad(img, o_hb + LD4, h->reward_h1_b.data, 1, 400, 1, 400, 400, (int)LD4);
    pol_pad(img, o_out, h->reward_hout_w.data, 400, 1, 1, 1, 1, (int)LDS);
    pol_pad(img, o_outb, h->reward_hout_b.data, 1, 1, 1, 1, 1, (int)LDS);
    HIP_TRY(hipSetDevice(env->cfg.device));
    if (!env->pol_heads_mem) HIP_TRY(hipMalloc((void **)&env->pol_heads_mem, at * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(env->pol_heads_mem, img.data(), at * sizeof(float), hipMemcpyHostToDevice, env->stream));
    HIP_TRY(hipStreamSynchronize(env->stream));             // (the staging vector goes out of scope)
    const float *m = env->pol_heads_mem;
    RcImagineDev &d = env->pol_i;
    d.rh_w[0] = m + o_h0; d.rh_w[1] = m + o_h1; d.rh_b[0] = m + o_hb; d.rh_b[1] = m + o_hb + LD4; d.rout_w = m + o_out; d.rout_b = m + o_outb;
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
    if (a->slot_mask == 0) return fail(RC_ERR_INVALID, "rc_policy_imagine: the slot mask is empty");
    if (a->slot_mask >> env->cfg.cars_per_env)
        return fail(RC_ERR_INVALID, "rc_policy_imagine: slot mask 0x%x names slots beyond cars_per_env = %d", a->slot_mask, env->cfg.cars_per_env);
    if (!a->reward && !a->actions && !a->features && !a->reward_start) return fail(RC_ERR_INVALID, "rc_policy_imagine: no output asked for");
    if ((a->reward || a->reward_start) && !env->pol_i.rout_w)
        return fail(RC_ERR_INVALID, "rc_policy_imagine: a reward is asked for and no reward head is loaded (rc_policy_load_heads)");
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcImagineCall c{};
    c.w = env->pol;
    c.ws = env->pol_s;
    c.wi = env->pol_i;
    c.state = env->pol_state;
    c.episode = env->params.st.episode;
    c.agent_steps = env->params.st.agent_steps;
    c.seed_lo = seed_lo(a->seed); c.seed_hi = seed_hi(a->seed);
    c.first_env = env->params.first_env;
    c.cars_per_env = env->cfg.cars_per_env;
    for (int s = 0; s < env->cfg.cars_per_env; ++s)
        if ((a->slot_mask >> s) & 1u) c.slots |= (uint32_t)s << (8 * c.n_slots++);
    c.n_active = env->cfg.num_envs * c.n_slots;
    c.horizon = a->horizon;
    c.sample = a->mode == RC_POLICY_IMAGINE_SAMPLE;
    c.actions_in = a->actions_in;
    c.reward = a->reward; c.actions = a->actions; c.features = a->features; c.reward_start = a->reward_start;
    KernelTimer t;
    int rc = t.begin(env, RC_K_POLICY);
    if (rc) return rc;
    hipEvent_t ea = nullptr, eb = nullptr;
    rck_take_launch_events(&ea, &eb);
    HIP_TRY(rck_launch_imagine(c, ea, eb, env->stream));
    return t.end();
}

}  // extern "C"
