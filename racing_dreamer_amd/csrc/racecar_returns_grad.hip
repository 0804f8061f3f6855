// rc_policy_returns_grad: the gradient of the reference's actor loss through the dream (dreamer/models.py:113-128 in `Dreamer.train`;
// DESIGN.md §2 item 26) - rc_policy_returns' rollout, then the adjoint of the lambda-return and the vector-Jacobian product of the
// three heads and of RSSM.img_step back to the actions and to the start latent, in the binary32 arithmetic of
// tests/policy_returns_grad_spec.c; the device equals it bit for bit.  The actor is not differentiated: the reference feeds it
// stop_gradient(feat) (models.py:218-219), so the cotangent of a feature reaches the actor's weights only through the action that
// enters img_step, and the closed-loop backward pass is the open-loop one under the actions the actor produced.  What leaves are
// the rows rc_policy_actor_fit_step consumes: the feature the actor read, the normals of its draw, the cotangent on its action.
// No weight gradient, no reduction across rows, no atomics: rows are independent.
//
// ONE kernel per mode, one launch per chunk of rows; the geometry is rc_policy_returns_kernel's (32 rows per workgroup, four waves,
// X and Y [32][417] and the latent Z [32][233] in LDS, the layers of racecar_rollout.h, the two series in[t] and g[t] behind them).
//   forward   item 20's step and recursion, unchanged in arithmetic, draws and keying (tag 5 for live rows, tag 8 for state rows).
//             What the backward needs of step t goes to the row's stash in global memory as the layer that made it is read by the
//             next: per (row, t) RC_RETURNS_GRAD_STASH floats = item 23's record 2 240 | a1, a2, a3 of the value head 1 200 | of the
//             pcont head 1 200 | v, p, weight, R and the three coefficients 8.  A workgroup reads back only what its own waves wrote,
//             a barrier later.
//   adjoint   thread `row` runs the recursion for R, then A_t and the coefficients c_r, c_v and the pcont logit's delta in ascending
//             t, from the row's series staged in X; they go to the row's stash (three [H][32] series do not fit in LDS beside the
//             sampled kernel's draws at H = 64).
//   backward  t = H - 1 .. 0 on the same tiles; Z holds the carry (deter 200 | stoch 30).  Each head that has a coefficient at t
//             is seeded with its row's own, carried through its layers' transposed images and added into the carry - reward,
//             value, pcont, one addition each - then the prior step (racecar_dream_grad.h).  The normals of `sample` mode are drawn
//             again from the step's key.
// The host cuts the rows into chunks against the handle's stash (returns_grad_run): a row's numbers depend on nothing but the row.
#include "racecar_dream_grad.h"

#define RC_RETURNS_GRAD_STASH 4648

namespace {

constexpr int RW = RC_RETURNS_GRAD_STASH;
// behind item 23's record: the value head's and the pcont head's activations, then the row's series at step t
enum { S_VA1 = RC_DREAM_GRAD_STASH, S_VA2 = S_VA1 + 400, S_VA3 = S_VA2 + 400, S_PA1 = S_VA3 + 400, S_PA2 = S_PA1 + 400, S_PA3 = S_PA2 + 400,
       S_SER = S_PA3 + 400 };
enum { Q_V = 0, Q_P, Q_W, Q_R, Q_CR, Q_CV, Q_DP };                    // the series' slots: Q_CR .. Q_DP are the three seeds of step t
static_assert(S_SER + 8 == RW, "the record of one row and step");

// behind X, Y, Z: the row's index in the caller's arrays (int64, -1 past the end), r | v | p of the step (backward: the three seeds),
// the two series; sampled: the draw's key and a step's normals - rc_policy_returns_kernel's budget
__host__ __device__ constexpr int rg_series_floats(int horizon) { return 2 * PM * (horizon - 1); }
constexpr size_t rg_lds_bytes(int horizon, bool sampled) {
    return RO_LDS_XYZ + PM * (sizeof(int64_t) + 3 * sizeof(float)) + (size_t)rg_series_floats(horizon) * sizeof(float) + (sampled ? RO_LDS_DRAWS : 0);
}
static_assert(rg_lds_bytes(RC_POLICY_IMAGINE_MAX_HORIZON, true) <= 160 * 1024, "the sampled kernel's LDS at the longest horizon");
static_assert(4 * RC_POLICY_IMAGINE_MAX_HORIZON * PM <= PM * XS, "X stages a row's four series for the adjoint");

enum { GK_STOCH = RO_OUT, GK_ACTION, GK_REWARD, GK_VALUE, GK_PCONT };

// delta of a head's last hidden layer -> X: fmaf(seed of the row, out_w[j], 0) elu'(a[j]).  (A thread asks for the stash entries of
// U elements before it uses the first, as racecar_dream_grad.hip's step 1.)
__device__ __forceinline__ void rg_seed(float *X, const float *seed, const float *out_w, const float *act, size_t stride, int tid) {
    constexpr int U = 10;
    static_assert(PM * RC_POLICY_UNITS % (PT * U) == 0, "whole batches");
#pragma unroll 1
    for (int base = tid; base < PM * RC_POLICY_UNITS; base += PT * U) {
        float a[U], wo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + u * PT, row = idx / RC_POLICY_UNITS, j = idx - row * RC_POLICY_UNITS;
            a[u] = act[row * stride + j];
            wo[u] = out_w[(size_t)j * RC_POLICY_LDSMALL];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + u * PT, row = idx / RC_POLICY_UNITS, j = idx - row * RC_POLICY_UNITS;
            X[row * XS + j] = fmaf(seed[row], wo[u], 0.0f) * dg_elu_grad(a[u]);
        }
    }
}

// A head's feature gradient added into the carry: the seed's delta in X, through the transposed images of its hidden layers
// (t[n_hidden - 1] .. t[1], [400][416]) and of its first layer (t[0], [400][256]); a[l] = the stashed activation of layer l (row
// 0's).  N_HIDDEN + 1 barriers, the first in front of the first product, the last behind the addition.
template <int N_HIDDEN>
__device__ __forceinline__ void rg_head_back(float *X, float *Y, float *Z, const float *const (&t)[N_HIDDEN], const float *const (&a)[N_HIDDEN],
                                             size_t stride, int wave, int lane) {
    float *src = X, *dst = Y;
#pragma unroll
    for (int l = N_HIDDEN - 1; l >= 1; --l) {
        __syncthreads();
        const float *al = a[l - 1];
        dg_layer400(src, RC_POLICY_UNITS, t[l], wave, lane, [&](int row, int j, float v) { dst[row * XS + j] = v * dg_elu_grad(al[row * stride + j]); });
        float *tmp = src;
        src = dst;
        dst = tmp;
    }
    __syncthreads();
    // carry = g_head + carry, in place (feature column j: stoch | deter)
    dg_layer256(src, RC_POLICY_UNITS, nullptr, 0, t[0], FEAT, wave, lane, [&](int row, int j, float v) {
        float *z = Z + row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH);
        *z = v + *z;
    });
    __syncthreads();
}

template <bool SAMPLED>
__device__ __forceinline__ void rg_returns_grad(const RcReturnsGradCall &g) {
    extern __shared__ float rg_lds[];
    const RcReturnsCall &c = g.r;
    const int H = c.horizon;
    const RoLds lds = ro_carve(rg_lds);
    float *X = lds.X, *Y = lds.Y, *Z = lds.Z;
    int64_t *out_row = (int64_t *)lds.rest;                  // [32] the row's index in the caller's arrays, -1 past the end
    float *cur = (float *)(out_row + PM);                    // [3][32] r, v, p of the step; backward: c_r, c_v and the logit delta
    float *s_in = cur + 3 * PM;                              // [H - 1][32]  in[t]
    float *s_g = s_in + rg_series_floats(H) / 2;             // [H - 1][32]  g[t] = p[t] lambda
    uint32_t *key = (uint32_t *)(s_g + rg_series_floats(H) / 2);      // [32][4]   (sampled only)
    float *normals = (float *)(key + 4 * PM);                // [32][PN]  (sampled only)
    const int tid = threadIdx.x;
    const int64_t row0 = g.row_begin + (int64_t)blockIdx.x * PM;
    const size_t stride = (size_t)H * RW;                    // a row's stash
    float *stash = g.stash + (size_t)blockIdx.x * PM * stride;

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
    ro_load_latent_rows(c.state, [&](int row) { return out_row[row]; }, Z, tid);
    __syncthreads();

    const bool open_loop = c.actions_in != nullptr, pcont_head = c.wc.pout_w != nullptr;
    auto stage_normals = [&](int t, bool with_action) {
        ro_stage_normals(normals, [&](int row) { return out_row[row] >= 0; }, [&](int row, uint32_t blk, float (&n)[4]) {
            const uint32_t *k = key + 4 * row;
            if (c.live) pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, blk, c.rows.seed_lo, c.rows.seed_hi, n);
            else pm_returns_normal_block(k[0], k[1], (uint32_t)t, blk, c.seed_lo, c.seed_hi, n);
        }, with_action, tid);
    };

    // ---- forward: racecar_returns.hip's loop; from t = 0 on every head runs wherever the recursion or an output reads it
    const bool start = c.reward_start || c.value_start || c.pcont_start;
    const float one_minus_lambda = 1.0f - c.lambda;
    float r_prev = 0.0f, p_prev = 0.0f, weight = 1.0f;       // of thread `row` (tid < 32)
#pragma unroll 1
    for (int t = start ? -1 : 0; t < H; ++t) {
        float *st = stash + (size_t)(t < 0 ? 0 : t) * RW;    // (t < 0 keeps nothing)
        // (the thread's index, opaque per step: see the backward loop)
        int td = tid;
        asm volatile("" : "+v"(td));
        const int wv = td >> 6, ln = td & 63;
        auto at_step = [&](int row) { return out_row[row] >= 0 ? out_row[row] * H + t : (int64_t)-1; };
        if (t >= 0) {
            if constexpr (SAMPLED) stage_normals(t, !open_loop);
            if (open_loop) ro_stage_actions(c.actions_in, c.actions, at_step, Z, td);
            // the feature the actor reads for a_t: the latent as the step finds it
            if (g.actor_features) ro_store_features(g.actor_features, at_step, Z, td);
            __syncthreads();
            if constexpr (SAMPLED) {
                if (g.eps && td < 2 * PM) {
                    const int row = td >> 1, j = td & 1;
                    const int64_t q = at_step(row);
                    if (q >= 0) g.eps[(size_t)q * 2 + j] = normals[row * PN + 32 + j];
                }
            }
        }
        const bool inner = t < H - 1;
        const bool run_actor = t >= 0 && !open_loop, run_prior = t >= 0;
        const bool run_reward = t < 0 ? c.reward_start != nullptr : (c.reward != nullptr || inner);
        const bool run_value = t < 0 ? c.value_start != nullptr : true;
        const bool run_pcont = t < 0 ? c.pcont_start != nullptr : (pcont_head && (c.pcont != nullptr || inner));
        // mode `mean`: tanh of the actor's mean; a head's one column (t < 0: the starting feature) stays in `cur` for the fold
        auto out = [&](const RoLayer &L, int row, int j, float v) {
            const int64_t q = out_row[row];
            if (L.kind == GK_ACTION) {
                const float *hn = c.w.hnorm;
                const float act = hn ? pm_action_normalized(v, hn[j], hn[2 + j], hn[4 + j], hn[6 + j]) : pm_action_plain(v);
                L.d[row * ZS + j] = act;
                if (q >= 0 && c.actions) c.actions[((size_t)q * H + t) * 2 + j] = act;
            } else {
                const float o = L.kind == GK_PCONT ? pm_sigmoid(v) : v;          // Bernoulli(logits).mean()
                cur[(L.kind - GK_REWARD) * PM + row] = o;
                if (q >= 0 && L.g) L.g[t < 0 ? (size_t)q : (size_t)q * H + t] = o;
            }
        };
#pragma unroll 1
        for (int layer = 0; layer < 19; ++layer) {
            const bool run = layer < 5 ? run_actor : (layer < 8 ? run_prior : (layer < 11 ? run_reward : (layer < 15 ? run_value : run_pcont)));
            if (!run) continue;
            RoLayer L;
            switch (layer) {
            case 0: L = ro_first(Z, c.w.h_w[0], c.w.h_b[0], X); break;
            case 1: L = ro_hidden(X, c.w.h_w[1], c.w.h_b[1], Y); break;
            case 2: L = ro_hidden(Y, c.w.h_w[2], c.w.h_b[2], X); break;
            case 3: L = ro_hidden(X, c.w.h_w[3], c.w.h_b[3], Y); break;
            case 4: L = ro_actor_out<SAMPLED>(Y, c.w, c.ws, Z, GK_ACTION); break;
            case 5: L = ro_img1(Z, c.w, X); break;
            case 6: L = ro_img2(Y, c.wi, X); break;
            case 7: L = ro_img3(X, c.wi, Z, SAMPLED ? GK_STOCH : RO_STORE_Z); break;
            case 8: L = ro_first(Z, c.wi.rh_w[0], c.wi.rh_b[0], X); break;
            case 9: L = ro_hidden(X, c.wi.rh_w[1], c.wi.rh_b[1], Y); break;
            case 10: L = ro_column(Y, c.wi.rout_w, c.wi.rout_b, GK_REWARD, t < 0 ? c.reward_start : c.reward); break;
            case 11: L = ro_first(Z, c.wc.vh_w[0], c.wc.vh_b[0], X); break;
            case 12: L = ro_hidden(X, c.wc.vh_w[1], c.wc.vh_b[1], Y); break;
            case 13: L = ro_hidden(Y, c.wc.vh_w[2], c.wc.vh_b[2], X); break;
            case 14: L = ro_column(X, c.wc.vout_w, c.wc.vout_b, GK_VALUE, t < 0 ? c.value_start : c.value); break;
            case 15: L = ro_first(Z, c.wc.ph_w[0], c.wc.ph_b[0], X); break;
            case 16: L = ro_hidden(X, c.wc.ph_w[1], c.wc.ph_b[1], Y); break;
            case 17: L = ro_hidden(Y, c.wc.ph_w[2], c.wc.ph_b[2], X); break;
            default: L = ro_column(X, c.wc.pout_w, c.wc.pout_b, GK_PCONT, t < 0 ? c.pcont_start : c.pcont); break;
            }
            if (layer == 6) ro_commit_deter(Y, Z, td);
            if (t >= 0) {
                // the input of this layer is what the layer before left: kept while it is read
                if (layer == 7) dg_keep(X, XS, RC_POLICY_DETER, st + S_X2, stride, td);
                if (layer == 9) dg_keep(X, XS, RC_POLICY_UNITS, st + S_A1, stride, td);
                if (layer == 10) dg_keep(Y, XS, RC_POLICY_UNITS, st + S_A2, stride, td);
                if (layer == 12) dg_keep(X, XS, RC_POLICY_UNITS, st + S_VA1, stride, td);
                if (layer == 13) dg_keep(Y, XS, RC_POLICY_UNITS, st + S_VA2, stride, td);
                if (layer == 14) dg_keep(X, XS, RC_POLICY_UNITS, st + S_VA3, stride, td);
                if (layer == 16) dg_keep(X, XS, RC_POLICY_UNITS, st + S_PA1, stride, td);
                if (layer == 17) dg_keep(Y, XS, RC_POLICY_UNITS, st + S_PA2, stride, td);
                if (layer == 18) dg_keep(X, XS, RC_POLICY_UNITS, st + S_PA3, stride, td);
            }
            if (SAMPLED && (layer == 4 || layer == 7)) {
                if (wv == 0) ro_dense_pair(L, ln, [&](int row, int j, float mean, float raw) {
                    float v;
                    if (L.kind == GK_STOCH) {
                        v = ro_sampled_stoch(mean, raw, normals[row * PN + j]);
                        st[row * stride + S_RAW + j] = raw;
                    } else {
                        float mu, sd;
                        pm_actor_dist(mean, raw, c.ws.hnorm4, j, mu, sd);
                        v = pm_tanh(fmaf(sd, normals[row * PN + 32 + j], mu));
                        const int64_t q = out_row[row];
                        if (q >= 0 && c.actions) c.actions[((size_t)q * H + t) * 2 + j] = v;
                    }
                    L.d[row * ZS + j] = v;
                });
            } else ro_layer(L, wv, ln, out);
            __syncthreads();
            if (layer != 5) continue;
            dg_keep(X, XS, RC_POLICY_DETER, st + S_X1, stride, td);
            dg_keep(Z, ZS, RC_POLICY_DETER, st + S_H, stride, td);
            dg_gru(c.w, X, Z, Y, st, stride, wv, ln);
            __syncthreads();
        }
        if (t < 0) continue;
        if (c.features) ro_store_features(c.features, at_step, Z, tid);
        // thread `row` folds the step into the series (the heads' next writes to `cur` are a barrier away) and keeps v, p and the weight
        if (tid < PM) {
            const int64_t q = out_row[tid];
            const float v = cur[PM + tid], p = pcont_head ? cur[2 * PM + tid] : c.discount;
            if (!pcont_head && c.pcont && q >= 0) c.pcont[(size_t)q * H + t] = p;
            if (t >= 1) s_in[(t - 1) * PM + tid] = fmaf(p_prev * v, one_minus_lambda, r_prev);
            if (inner) s_g[t * PM + tid] = p * c.lambda;
            r_prev = cur[tid];
            p_prev = p;
            float *ser = st + tid * stride + S_SER;
            ser[Q_V] = v;
            ser[Q_P] = p;
            ser[Q_W] = weight;
            if (inner) {
                if (c.weight && q >= 0) c.weight[(size_t)q * (H - 1) + t] = weight;
                weight = weight * p;
            }
        }
    }
    if (!g.grad_actions && !g.grad_state && !c.returns) return;
    __syncthreads();

    // ---- the adjoint of the recursion.  X <- the rows' v, p, weight [3][H][32], all threads; then one lane per row.
    float *xv = X, *xp = X + H * PM, *xw = X + 2 * H * PM, *xr = X + 3 * H * PM;
    for (int idx = tid; idx < 3 * H * PM; idx += PT) {
        const int row = idx % PM, rest = idx / PM, t = rest % H, which = rest / H;
        X[idx] = stash[row * stride + (size_t)t * RW + S_SER + which];
    }
    __syncthreads();
    if (tid < PM) {
        const int64_t q = out_row[tid];
        float ret = xv[(H - 1) * PM + tid];                  // R[H - 1] = v[H - 1]
        xr[(H - 1) * PM + tid] = ret;
#pragma unroll 1
        for (int t = H - 2; t >= 0; --t) {
            ret = fmaf(s_g[t * PM + tid], ret, s_in[t * PM + tid]);
            if (c.returns && q >= 0) c.returns[(size_t)q * (H - 1) + t] = ret;
            xr[t * PM + tid] = ret;
        }
        float *ser = stash + tid * stride + S_SER;
        float A = 0.0f, p = 0.0f;
#pragma unroll 1
        for (int t = 0; t <= H - 2; ++t) {
            const float s = g.scale * xw[t * PM + tid];
            A = t == 0 ? s : fmaf(A, s_g[(t - 1) * PM + tid], s);
            p = xp[t * PM + tid];
            const float c_p = A * fmaf(c.lambda, xr[(t + 1) * PM + tid], xv[(t + 1) * PM + tid] * one_minus_lambda);
            ser[(size_t)t * RW + Q_CR] = A;
            ser[(size_t)t * RW + Q_DP] = c_p * (p * (1.0f - p));
            ser[(size_t)(t + 1) * RW + Q_CV] = (A * p) * one_minus_lambda;
        }
        ser[(size_t)(H - 1) * RW + Q_CV] = fmaf(A, s_g[(H - 2) * PM + tid], (A * p) * one_minus_lambda);
    }
    if (!g.grad_actions && !g.grad_state) return;

    // ---- backward: Z = the carry, deter at [0, 200), stoch at [200, 230)
    for (int idx = tid; idx < PM * ZS; idx += PT) Z[idx] = 0.0f;
    const float *const rt[2] = {g.wt.p.rh0_t, g.wt.p.rh1_t};
    const float *const vt[3] = {g.wt.vh_t[0], g.wt.vh_t[1], g.wt.vh_t[2]}, *const pt[3] = {g.wt.ph_t[0], g.wt.ph_t[1], g.wt.ph_t[2]};
    __syncthreads();                                         // (the coefficients are written, the carry is zero)
#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        const float *st = stash + (size_t)t * RW;            // (the step before is seven barriers through with `cur`)
        // (the thread's index and the row stride, opaque per step: the LDS and stash addresses of every epilogue below depend on
        // them alone, and are otherwise all computed in front of the loop and held across it - more of them than there are registers)
        int td = tid;
        size_t sd = stride;
        asm volatile("" : "+v"(td), "+s"(sd));
        const int wv = td >> 6, ln = td & 63;
        if (td < 3 * PM) {
            const int which = td / PM, row = td - which * PM;
            cur[td] = st[row * sd + S_SER + Q_CR + which];
        }
        if constexpr (SAMPLED) stage_normals(t, false);
        __syncthreads();
        // 1. the heads, each added head first: reward, value, pcont
        if (t < H - 1) {
            const float *const a[2] = {st + S_A1, st + S_A2};
            rg_seed(X, cur, c.wi.rout_w, a[1], sd, td);
            rg_head_back<2>(X, Y, Z, rt, a, sd, wv, ln);
        }
        if (t >= 1) {
            const float *const a[3] = {st + S_VA1, st + S_VA2, st + S_VA3};
            rg_seed(X, cur + PM, c.wc.vout_w, a[2], sd, td);
            rg_head_back<3>(X, Y, Z, vt, a, sd, wv, ln);
        }
        if (pcont_head && t < H - 1) {
            const float *const a[3] = {st + S_PA1, st + S_PA2, st + S_PA3};
            rg_seed(X, cur + 2 * PM, c.wc.pout_w, a[2], sd, td);
            rg_head_back<3>(X, Y, Z, pt, a, sd, wv, ln);
        }
        // 3-7. the prior step; a given raw action outside [-1, 1] has gradient +0 (the clamp); the actor's own lies inside
        dg_prior_back<SAMPLED>(g.wt.p, X, Y, Z, st, sd, normals, td, [&](int row, int j, float v) {
            const int64_t q = out_row[row];
            if (q < 0 || !g.grad_actions) return;
            const size_t at = ((size_t)q * H + t) * 2 + j;
            if (open_loop) {
                const float a = c.actions_in[at];
                v = (a >= -1.0f && a <= 1.0f) ? v : 0.0f;
            }
            g.grad_actions[at] = v;
        });
    }
    if (g.grad_state) ro_store_features(g.grad_state, [&](int row) { return out_row[row]; }, Z, tid);
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_returns_grad_kernel(RcReturnsGradCall g) { rg_returns_grad<false>(g); }
__global__ __launch_bounds__(PT) void rc_policy_returns_grad_sampled_kernel(RcReturnsGradCall g) { rg_returns_grad<true>(g); }

hipError_t rck_returns_grad_prepare() {
    return ro_prepare(rc_policy_returns_grad_kernel, rc_policy_returns_grad_sampled_kernel, rg_lds_bytes(RC_POLICY_IMAGINE_MAX_HORIZON, false),
                      rg_lds_bytes(RC_POLICY_IMAGINE_MAX_HORIZON, true));
}

// ---- the handle's images and stash, and the chunks of a call
struct RcReturnsGrad {
    float *images = nullptr;                   // the thirteen transposed images, one allocation
    RcReturnsGradDev wt{};
    bool pcont = false;                        // the pcont head's three are among them
    float *stash = nullptr;
    size_t stash_floats = 0;
};

namespace {

constexpr size_t kStashBudget = (size_t)1 << 30;          // bytes: the stash never grows beyond it (racecar_dream_grad.hip's)

struct TImage { int k_n, n, dst_ld, src_ld, group, group_ld; uint32_t head; };

}  // namespace

int returns_grad_release(rc_env *env) {
    env->rgrad_stale = 0;
    if (!env->rgrad) return RC_OK;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    if (env->rgrad->images) (void)hipFree(env->rgrad->images);
    if (env->rgrad->stash) (void)hipFree(env->rgrad->stash);
    delete env->rgrad;
    env->rgrad = nullptr;
    return RC_OK;
}

int returns_grad_run(rc_env *env, RcReturnsGradCall &c, int64_t chunk_rows) {
    const int D = RC_POLICY_DETER, U = RC_POLICY_UNITS, NS = RC_POLICY_STOCH;
    constexpr int N = 13;
    const TImage first{U, FEAT, LDT, RC_POLICY_LD400, U, 0, 0}, hidden{U, U, RC_POLICY_LD400, RC_POLICY_LD400, U, 0, 0};
    TImage table[N] = {
        {D, 32, 32, RC_POLICY_LD200, D, 0, 0},                                  // img1
        {3 * D, D, LDT, RC_POLICY_LDGRU, D, RC_POLICY_LD200, 0},                // gru_k
        {3 * D, D, LDT, RC_POLICY_LDGRU, D, RC_POLICY_LD200, 0},                // gru_r
        {D, D, LDT, RC_POLICY_LD200, D, 0, 0},                                  // img2
        {2 * NS, D, LDT, RC_POLICY_LDPAIR, NS, 32, 0},                          // img3
        first, hidden, first, hidden, hidden, first, hidden, hidden,            // reward, value, pcont
    };
    for (int i = 5; i < N; ++i) table[i].head = i < 7 ? RC_RGRAD_REWARD : (i < 10 ? RC_RGRAD_VALUE : RC_RGRAD_PCONT);
    const bool pcont = env->pol_c.pout_w != nullptr;
    const float *src[N] = {env->pol.img1_w, env->pol.gru_k, env->pol.gru_r, env->pol_i.img2_w, env->pol_i.img3_w, env->pol_i.rh_w[0], env->pol_i.rh_w[1],
                           env->pol_c.vh_w[0], env->pol_c.vh_w[1], env->pol_c.vh_w[2], env->pol_c.ph_w[0], env->pol_c.ph_w[1], env->pol_c.ph_w[2]};
    auto transpose = [&](int i, float *dst) {
        const TImage &im = table[i];
        rck_dream_grad_transpose(src[i], im.src_ld, im.group, im.group_ld, im.k_n, im.n, im.dst_ld, dst, env->stream);
    };
    if (env->rgrad && env->rgrad->pcont != pcont) {          // (the critic's loaders release: a guard, not a path)
        const int rc = returns_grad_release(env);
        if (rc) return rc;
    }
    if (!env->rgrad) {
        // the first call after the weights were loaded: the transposed images, built on the device
        size_t at[N], total = 0;
        for (int i = 0; i < N; ++i) {
            at[i] = total;
            total += ((size_t)table[i].k_n * table[i].dst_ld + 63) / 64 * 64;
        }
        RcReturnsGrad *d = new RcReturnsGrad();
        const hipError_t e = hipMalloc((void **)&d->images, total * sizeof(float));
        if (e != hipSuccess) {
            delete d;
            return fail(RC_ERR_HIP, "rc_policy_returns_grad: %s", hipGetErrorString(e));
        }
        env->rgrad = d;
        d->pcont = pcont;
        const float **dst[N] = {&d->wt.p.img1_t, &d->wt.p.gruk_t, &d->wt.p.grur_t, &d->wt.p.img2_t, &d->wt.p.img3_t, &d->wt.p.rh0_t, &d->wt.p.rh1_t,
                                &d->wt.vh_t[0], &d->wt.vh_t[1], &d->wt.vh_t[2], &d->wt.ph_t[0], &d->wt.ph_t[1], &d->wt.ph_t[2]};
        for (int i = 0; i < N; ++i) {
            if (i >= 10 && !pcont) continue;                 // (null: the kernel does not read them)
            transpose(i, d->images + at[i]);
            *dst[i] = d->images + at[i];
        }
        HIP_TRY(hipGetLastError());
    } else if (env->rgrad_stale) {
        // a fit step moved a head since: its images again, in place and in stream order behind that step
        RcReturnsGradDev &w = env->rgrad->wt;
        const float *img[N] = {nullptr, nullptr, nullptr, nullptr, nullptr, w.p.rh0_t, w.p.rh1_t, w.vh_t[0], w.vh_t[1], w.vh_t[2], w.ph_t[0], w.ph_t[1], w.ph_t[2]};
        for (int i = 5; i < N; ++i)
            if ((env->rgrad_stale & table[i].head) && img[i]) transpose(i, const_cast<float *>(img[i]));
        HIP_TRY(hipGetLastError());
    }
    env->rgrad_stale = 0;
    RcReturnsGrad &d = *env->rgrad;
    const int64_t n_rows = c.r.n_rows, H = c.r.horizon;
    const size_t row_floats = (size_t)H * RW;
    const int64_t padded = (n_rows + PM - 1) / PM * PM;        // n_rows < 2^31
    int64_t chunk = (int64_t)(kStashBudget / (row_floats * sizeof(float))) / PM * PM;          // H = 15: 3 840 rows; H = 64: 896
    if (chunk > padded) chunk = padded;
    if (chunk_rows > 0 && chunk_rows < chunk) chunk = (chunk_rows + PM - 1) / PM * PM;         // (below `chunk`: the rounding cannot overflow)
    const size_t need = (size_t)chunk * row_floats;
    if (need > d.stash_floats) {
        if (d.stash) {
            HIP_TRY(hipStreamSynchronize(env->stream));
            (void)hipFree(d.stash);
            d.stash = nullptr;
            d.stash_floats = 0;
        }
        const hipError_t e = hipMalloc((void **)&d.stash, need * sizeof(float));
        if (e != hipSuccess) return fail(RC_ERR_HIP, "rc_policy_returns_grad: the stash of %zu bytes: %s", need * sizeof(float), hipGetErrorString(e));
        d.stash_floats = need;
    }
    c.wt = d.wt;
    c.stash = d.stash;
    KernelTimer t;
    const int rc = t.begin(env, RC_K_POLICY, true);
    if (rc) return rc;
    const uint32_t lds = (uint32_t)rg_lds_bytes((int)H, c.r.sample != 0);
    for (int64_t begin = 0; begin < n_rows; begin += chunk) {
        RcReturnsGradCall k = c;
        k.row_begin = begin;
        k.r.n_rows = begin + chunk < n_rows ? begin + chunk : n_rows;
        const unsigned blocks = (unsigned)((k.r.n_rows - begin + PM - 1) / PM);
        if (c.r.sample) hipLaunchKernelGGL(rc_policy_returns_grad_sampled_kernel, dim3(blocks), dim3(PT), lds, env->stream, k);
        else hipLaunchKernelGGL(rc_policy_returns_grad_kernel, dim3(blocks), dim3(PT), lds, env->stream, k);
    }
    const hipError_t e = hipGetLastError();
    const int rc_end = t.end();                             // (also after a refused launch: the event pair goes back to the handle)
    if (e != hipSuccess) return fail(RC_ERR_HIP, "rc_policy_returns_grad: %s", hipGetErrorString(e));
    return rc_end;
}
