// rc_policy_returns: the forward half of the reference's behaviour learning (dreamer/models.py:113-133 in `Dreamer.train`): the
// imagination rollout of rc_policy_imagine with the reward head, the value head and the pcont head (models.py:301-318
// DenseDecoder) on every imagined feature, then the lambda-return (dreamer/tools.py:396-418 `lambda_return` through
// `static_scan(reverse=True)`) and the discount weights cumprod([1, pcont[:-2]]) - H steps and the recursion in one launch, in the
// binary32 arithmetic of DESIGN.md §2 item 20 (tests/policy_returns_spec.c is the CPU restatement).
//
// The workgroup geometry is rc_policy_imagine_kernel's (racecar_policy_tiles.h): four waves, 32 rows, activations in the two
// [32][417] buffers X and Y, the latent in Z [32][233] = deter 200 | stoch 30 | action 2 for the whole horizon.  A row is a start:
// a car of the mask (live latents, arrays indexed by car, rc_policy_imagine's draws) or a row of the caller's state (draws keyed
// by row_offset + row under a tag of their own).  Per imagined step, with one barrier after each layer:
//   actor  h0 Z->X, h1 X->Y, h2 Y->X, h3 X->Y, hout Y->Z.action          (skipped when the caller gives the actions)
//   prior  img1 Z->X, GRU (X, Z.deter)->Y, img2 Y->X (and Y->Z.deter), img3 X->Z.stoch
//   reward h0 Z->X, h1 X->Y, hout Y->r[t]
//   value  h0 Z->X, h1 X->Y, h2 Y->X, hout X->v[t]
//   pcont  h0 Z->X, h1 X->Y, h2 Y->X, hout X->sigmoid->p[t]              (each head only when an output needs it)
// A head's one output column belongs to one lane of wave 0, which leaves r[t], v[t], p[t] of its 16 rows in LDS; after the
// step's last barrier thread `row` folds them into the two series the backward recursion reads, in[t - 1] = fmaf(p[t - 1] v[t],
// 1 - lambda, r[t - 1]) and g[t] = p[t] lambda - both single roundings of the recursion as written, so [2][H - 1][32] floats
// carry what three [H][32] series would (DESIGN.md §4 has the budget: the three do not fit beside the sampled kernel's LDS at
// H = 64, the two do) - and advances the weight.  After the last step the same thread runs R = v[H - 1]; R = fmaf(g[t], R, in[t])
// for t = H - 2 .. 0.  Only the requested outputs leave the CU.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int ZS = 233;                        // row stride of Z (41 mod 64, odd: the 32 rows on 32 banks)
constexpr int Z_STOCH = RC_POLICY_DETER, Z_ACTION = RC_POLICY_DETER + RC_POLICY_STOCH;
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
// behind X, Y, Z: the row's index in the caller's arrays (int64, -1 past the end), r | v | p of the step, the two series
constexpr size_t kLdsFixed = (size_t)(2 * PM * XS + PM * ZS) * sizeof(float) + PM * (sizeof(int64_t) + 3 * sizeof(float));
constexpr size_t kLdsSampled = (size_t)PM * (PN + 4) * sizeof(float);                        // a step's normals and the draw's key
__host__ __device__ constexpr int rt_series_floats(int horizon) { return horizon > 1 ? 2 * PM * (horizon - 1) : 0; }
constexpr size_t rt_lds_bytes(int horizon, bool sampled) {
    return kLdsFixed + (size_t)rt_series_floats(horizon) * sizeof(float) + (sampled ? kLdsSampled : 0);
}
static_assert(rt_lds_bytes(64, true) <= 160 * 1024, "the sampled kernel's LDS at the longest horizon");

enum { RK_ELU = 0, RK_STOCH = 1, RK_ACTION = 2, RK_REWARD = 3, RK_VALUE = 4, RK_PCONT = 5 };

struct RtLayer {
    const float *a;          // LDS input, first column; rows `as` apart
    int k;
    const float *a2;         // second part of the input (weight rows k ..), or k2 = 0
    int k2, as;
    const float *w, *b;
    int ld, n;
    float *d;                // LDS output, first column; rows `ds` apart
    int ds, kind;
};

struct RtRows {
    const int64_t *out;      // [32] the row's index in the caller's arrays, -1 past the end
    float *cur;              // [3][32] r, v, p of the step
    const float *normals;    // [32][PN] (sampled only)
};

// One wave's tiles of a layer.  PAIR = false: the 32-column tiles at col0, col0 + 128, ...  PAIR = true (TN = 2, the sampled
// mode's img3 and hout): mean columns in tile 0, raw std columns in tile 1 of an ld-64 image.
template <int TN, bool PAIR>
__device__ __forceinline__ void rt_dense(const RcReturnsCall &c, const RtLayer &L, const RtRows &R, int t, int col0, int lane) {
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
            if (L.kind == RK_STOCH) {
                v = fmaf(pm_softplus(acc[1][r]) + PM_STOCH_MIN_STD, R.normals[row * PN + cc], acc[0][r]);
            } else {
                float mu, sd;
                pm_actor_dist(acc[0][r], acc[1][r], c.ws.hnorm4, cc, mu, sd);
                v = pm_tanh(fmaf(sd, R.normals[row * PN + 32 + cc], mu));
                const int64_t q = R.out[row];
                if (q >= 0 && c.actions) c.actions[((size_t)q * c.horizon + t) * 2 + cc] = v;
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
                if (L.kind == RK_ELU) {
                    L.d[row * L.ds + j] = pm_elu(v);
                } else if (L.kind == RK_STOCH) {           // mode `mean`: the prior's mean is the new stoch
                    L.d[row * L.ds + j] = v;
                } else if constexpr (TN == 1) {            // (the layers of one tile: the actor's output and the heads')
                    const int64_t q = R.out[row];
                    if (L.kind == RK_ACTION) {             // mode `mean`: tanh of the actor's mean
                        const float *hn = c.w.hnorm;
                        const float act = hn ? pm_action_normalized(v, hn[j], hn[2 + j], hn[4 + j], hn[6 + j]) : pm_action_plain(v);
                        L.d[row * L.ds + j] = act;
                        if (q >= 0 && c.actions) c.actions[((size_t)q * c.horizon + t) * 2 + j] = act;
                    } else if (q >= 0) {                   // a head's one column: t < 0 is the starting feature
                        const int which = L.kind - RK_REWARD;
                        const float o = L.kind == RK_PCONT ? pm_sigmoid(v) : v;      // Bernoulli(logits).mean()
                        R.cur[which * PM + row] = o;
                        float *dst;
                        if (t < 0) dst = which == 0 ? c.reward_start : (which == 1 ? c.value_start : c.pcont_start);
                        else dst = which == 0 ? c.reward : (which == 1 ? c.value : c.pcont);
                        if (dst) dst[t < 0 ? (size_t)q : (size_t)q * c.horizon + t] = o;
                    }
                }
            }
        }
    }
}

template <bool SAMPLED>
__device__ __forceinline__ void rt_returns(const RcReturnsCall &c) {
    extern __shared__ float rt_lds[];
    const int H = c.horizon;
    float *X = rt_lds, *Y = rt_lds + PM * XS, *Z = rt_lds + 2 * PM * XS;
    int64_t *out_row = (int64_t *)(Z + PM * ZS);             // [32]  (the floats before it are a multiple of 8 bytes)
    float *cur = (float *)(out_row + PM);                    // [3][32]
    float *s_in = cur + 3 * PM;                              // [H - 1][32]  in[t]
    float *s_g = s_in + rt_series_floats(H) / 2;             // [H - 1][32]  g[t] = p[t] lambda
    uint32_t *key = (uint32_t *)(s_g + rt_series_floats(H) / 2);      // [32][4]   (sampled only)
    float *normals = (float *)(key + 4 * PM);                // [32][PN]  (sampled only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PM;

    if (tid < PM) {
        const int64_t q = row0 + tid;
        int64_t o = -1;
        uint32_t k[4] = {0u, 0u, 0u, 0u};
        if (q < c.n_rows) {
            if (c.live) {
                // the car of row q of the mask's rows; its draws are rc_policy_imagine's: (global env, episode, agent step, slot)
                const int car = pm_car(c.rows, (int)q);
                o = car;
                const int e = car / c.rows.cars_per_env;
                k[0] = c.rows.first_env + (uint32_t)e;
                k[1] = c.rows.episode[e];
                k[2] = (uint32_t)c.rows.agent_steps[e];
                k[3] = (uint32_t)(car - e * c.rows.cars_per_env);
            } else {
                o = q;
                const uint64_t id = c.row_offset + (uint64_t)q;
                k[0] = (uint32_t)id;
                k[1] = (uint32_t)(id >> 32);
            }
        }
        out_row[tid] = o;
        cur[tid] = cur[PM + tid] = cur[2 * PM + tid] = 0.0f;
        if constexpr (SAMPLED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) key[4 * tid + i] = k[i];
        }
    }
    __syncthreads();
    // the latent of the row: stoch | deter of its state row (the two action columns are not read); zero rows past the end
    for (int idx = tid; idx < PM * ZS; idx += PT) {
        const int row = idx / ZS, j = idx - row * ZS;
        const int64_t l = out_row[row];
        float v = 0.0f;
        if (l >= 0 && j < FEAT) v = c.state[(size_t)l * RC_POLICY_STATE + (j < RC_POLICY_DETER ? RC_POLICY_STOCH + j : j - RC_POLICY_DETER)];
        Z[idx] = v;
    }
    __syncthreads();

    const RtRows R{out_row, cur, normals};
    const bool open_loop = c.actions_in != nullptr, pcont_head = c.wc.pout_w != nullptr;
    const bool start = c.reward_start || c.value_start || c.pcont_start;
    const float one_minus_lambda = 1.0f - c.lambda;
    float r_prev = 0.0f, p_prev = 0.0f, weight = 1.0f;       // of thread `row` (tid < 32)
#pragma unroll 1
    for (int t = start ? -1 : 0; t < H; ++t) {
        if (t >= 0) {
            if constexpr (SAMPLED) {
                // thread (row, block) = (tid / 8, tid % 8) draws block `block` of step t, the thread of block 0 also block 8
                const int row = tid >> 3, blk = tid & 7;
                const uint32_t *k = key + 4 * row;
                float n[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (out_row[row] >= 0) {
                    if (c.live) {
                        pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, (uint32_t)blk, c.rows.seed_lo, c.rows.seed_hi, n);
                        if (blk == 0 && !open_loop) pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, PM_BLOCK_ACTION, c.rows.seed_lo, c.rows.seed_hi, m);
                    } else {
                        pm_returns_normal_block(k[0], k[1], (uint32_t)t, (uint32_t)blk, c.seed_lo, c.seed_hi, n);
                        if (blk == 0 && !open_loop) pm_returns_normal_block(k[0], k[1], (uint32_t)t, PM_BLOCK_ACTION, c.seed_lo, c.seed_hi, m);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    normals[row * PN + 4 * blk + i] = n[i];
                    if (blk == 0) normals[row * PN + 32 + i] = m[i];
                }
            }
            if (open_loop && tid < 2 * PM) {
                const int row = tid >> 1, j = tid & 1;
                const int64_t q = out_row[row];
                const float a = q >= 0 ? pm_clamp_action(c.actions_in[((size_t)q * H + t) * 2 + j]) : 0.0f;
                Z[row * ZS + Z_ACTION + j] = a;
                if (q >= 0 && c.actions) c.actions[((size_t)q * H + t) * 2 + j] = a;
            }
            __syncthreads();
        }
        // what this step runs: the recursion reads r[t] and p[t] for t < H - 1 only, v[t] for all t
        const bool inner = t < H - 1;
        const bool run_actor = t >= 0 && !open_loop, run_prior = t >= 0;
        const bool run_reward = t < 0 ? c.reward_start != nullptr : (c.reward != nullptr || (c.returns != nullptr && inner));
        const bool run_value = t < 0 ? c.value_start != nullptr : (c.value != nullptr || c.returns != nullptr);
        const bool run_pcont = t < 0 ? c.pcont_start != nullptr : (pcont_head && (c.pcont != nullptr || ((c.returns != nullptr || c.weight != nullptr) && inner)));
#pragma unroll 1
        for (int layer = 0; layer < 19; ++layer) {
            const bool run = layer < 5 ? run_actor : (layer < 8 ? run_prior : (layer < 11 ? run_reward : (layer < 15 ? run_value : run_pcont)));
            if (!run) continue;
            RtLayer L;
            switch (layer) {
            case 0: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.w.h_w[0], c.w.h_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 1: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[1], c.w.h_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, RK_ELU}; break;
            case 2: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[2], c.w.h_b[2], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 3: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.w.h_w[3], c.w.h_b[3], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, RK_ELU}; break;
            case 4: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, SAMPLED ? c.ws.hout_w : c.w.hout_w, SAMPLED ? c.ws.hout_b : c.w.hout_b,
                         SAMPLED ? RC_POLICY_LDPAIR : RC_POLICY_LDSMALL, 2, Z + Z_ACTION, ZS, RK_ACTION}; break;
            case 5: L = {Z + Z_STOCH, 32, nullptr, 0, ZS, c.w.img1_w, c.w.img1_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, RK_ELU}; break;
            case 6: L = {Y, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img2_w, c.wi.img2_b, RC_POLICY_LD200, RC_POLICY_DETER, X, XS, RK_ELU}; break;
            case 7: L = {X, RC_POLICY_DETER, nullptr, 0, XS, c.wi.img3_w, c.wi.img3_b, RC_POLICY_LDPAIR, RC_POLICY_STOCH, Z + Z_STOCH, ZS, RK_STOCH}; break;
            case 8: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.wi.rh_w[0], c.wi.rh_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 9: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rh_w[1], c.wi.rh_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, RK_ELU}; break;
            case 10: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.wi.rout_w, c.wi.rout_b, RC_POLICY_LDSMALL, 1, nullptr, 0, RK_REWARD}; break;
            case 11: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.wc.vh_w[0], c.wc.vh_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 12: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.vh_w[1], c.wc.vh_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, RK_ELU}; break;
            case 13: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.vh_w[2], c.wc.vh_b[2], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 14: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.vout_w, c.wc.vout_b, RC_POLICY_LDSMALL, 1, nullptr, 0, RK_VALUE}; break;
            case 15: L = {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, c.wc.ph_w[0], c.wc.ph_b[0], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            case 16: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.ph_w[1], c.wc.ph_b[1], RC_POLICY_LD400, RC_POLICY_UNITS, Y, XS, RK_ELU}; break;
            case 17: L = {Y, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.ph_w[2], c.wc.ph_b[2], RC_POLICY_LD400, RC_POLICY_UNITS, X, XS, RK_ELU}; break;
            default: L = {X, RC_POLICY_UNITS, nullptr, 0, XS, c.wc.pout_w, c.wc.pout_b, RC_POLICY_LDSMALL, 1, nullptr, 0, RK_PCONT}; break;
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
                if (wave == 0) rt_dense<2, true>(c, L, R, t, 0, lane);
            } else if (mine == 1) rt_dense<1, false>(c, L, R, t, 32 * wave, lane);
            else if (mine == 2) rt_dense<2, false>(c, L, R, t, 32 * wave, lane);
            else if (mine == 3) rt_dense<3, false>(c, L, R, t, 32 * wave, lane);
            else if (mine == 4) rt_dense<4, false>(c, L, R, t, 32 * wave, lane);
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
        if (t < 0) continue;
        // feature[t] = [stoch', deter'] from the latent (its next writer is a barrier away)
        if (c.features) {
            for (int idx = tid; idx < PM * FEAT; idx += PT) {
                const int row = idx / FEAT, j = idx - row * FEAT;
                const int64_t q = out_row[row];
                if (q >= 0) c.features[((size_t)q * H + t) * FEAT + j] = Z[row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH)];
            }
        }
        // thread `row` folds the step into the series (the heads' next writes to `cur` are a barrier away)
        if (tid < PM && out_row[tid] >= 0) {
            const size_t q = (size_t)out_row[tid];
            const float p = pcont_head ? cur[2 * PM + tid] : c.discount;
            if (!pcont_head && c.pcont) c.pcont[q * H + t] = p;
            if (c.returns) {
                if (t >= 1) s_in[(t - 1) * PM + tid] = fmaf(p_prev * cur[PM + tid], one_minus_lambda, r_prev);
                if (inner) s_g[t * PM + tid] = p * c.lambda;
                r_prev = cur[tid];
                p_prev = p;
            }
            if (c.weight && inner) {
                c.weight[q * (H - 1) + t] = weight;
                weight = weight * p;
            }
        }
    }
    // the backward recursion, one lane per row, over what the same lane wrote
    if (c.returns && tid < PM && out_row[tid] >= 0) {
        const size_t q = (size_t)out_row[tid];
        float ret = cur[PM + tid];                           // R[H - 1] = v[H - 1]
#pragma unroll 1
        for (int t = H - 2; t >= 0; --t) {
            ret = fmaf(s_g[t * PM + tid], ret, s_in[t * PM + tid]);
            c.returns[q * (H - 1) + t] = ret;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_returns_kernel(RcReturnsCall c) { rt_returns<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_returns_sampled_kernel(RcReturnsCall c) { rt_returns<true>(c); }

hipError_t rck_returns_prepare() {
    const hipError_t e = hipFuncSetAttribute((const void *)rc_policy_returns_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)rt_lds_bytes(RC_POLICY_IMAGINE_MAX_HORIZON, false));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)rc_policy_returns_sampled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)rt_lds_bytes(RC_POLICY_IMAGINE_MAX_HORIZON, true));
}

hipError_t rck_launch_returns(const RcReturnsCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.n_rows + PM - 1) / PM);
    const uint32_t lds = (uint32_t)rt_lds_bytes(c.horizon, c.sample != 0);
    if (!c.sample) hipExtLaunchKernelGGL(rc_policy_returns_kernel, dim3(blocks), dim3(PT), lds, s, start, stop, 0u, c);
    else hipExtLaunchKernelGGL(rc_policy_returns_sampled_kernel, dim3(blocks), dim3(PT), lds, s, start, stop, 0u, c);
    return hipGetLastError();
}
