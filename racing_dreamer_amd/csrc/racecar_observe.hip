// rc_policy_observe: the reference's posterior chain over RECORDED sequences (dreamer/models.py:325-336 `RSSM.observe`; with
// context < length followed by `RSSM.imagine` under the recorded actions, the "observe K, dream the rest" of models.py:243-277
// `_image_summaries`), its KL term (models.py:84-110 `_train`: kl_divergence(post, prior)) and the reward head on the features,
// T steps of N recorded windows in one launch, in the binary32 arithmetic of DESIGN.md §2 item 17 (tests/policy_observe_spec.c
// is the CPU restatement).
//
// The workgroup geometry is rc_policy_imagine_kernel's (racecar_policy_tiles.h): four waves, 32 rows (a row is one window, not
// a car of the env), activations in the two [32][417] buffers X and Y, the latent in Z [32][233] = deter 200 | stoch 30 | action 2
// for all T steps.  Per observed step, with one barrier after each:
//   prior      img1 Z->X, GRU (X, Z.deter)->Y, img2 Y->X (and Y->Z.deter), img3 X->(mean, raw std) in X[256, 320); all threads:
//              std, the outputs, past the context stoch' into Z
//   posterior  obs1 on [Z.deter, scan[row, t] staged through X[0, 120) in 9 pieces]->Y, obs2 Y->(mean, raw std) in Y[256, 320);
//              all threads: std, the outputs, stoch' into Z, the KL's 30 terms per row into Y[320, 350); one thread per row
//              sums them ascending                                                                   (t < context only)
//   head       h0 Z->X, h1 X->Y, hout Y->reward[t]                                 (skipped when no reward is asked for)
// obs2 and img3 read their ld-64 pair images (mean columns in tile 0, raw std in tile 1) in both modes, on one wave; their
// softplus and the KL's logarithms are spread over the four waves, and the softplus of a std nobody asked for is not taken.  Only the requested outputs leave the CU.  DESIGN.md §4 has the LDS budget.
#include "racecar_env.h"
#include "racecar_rollout.h"

namespace {

constexpr int SCK = 120;                       // beams per staged piece of the scan (9 pieces), as rc_policy_kernel's
constexpr int N_BEAMS = 1080;
// columns of X (img3: the prior, kept until obs2's KL of the same step) and of Y (obs2: the posterior) behind the activations
constexpr int P_MEAN = 256, P_STD = 288;       // [256, 286) the mean, [288, 318) the raw std, then the std
constexpr int P_KL = 320;                      // Y[320, 350) the KL's terms of a row
constexpr size_t kLdsBytes = RO_LDS_XYZ;
constexpr size_t kLdsBytesSampled = kLdsBytes + (size_t)PM * PN * sizeof(float);             // + a step's normals

enum { OK_REWARD = RO_OUT };

// img3 (POST = false, input X) and obs2 (POST = true, input Y) on one wave: the mean columns (tile 0) and the raw std columns
// (tile 1) of the ld-64 pair image into columns [256, 288) and [288, 320) of the buffer the layer read
template <bool POST>
__device__ __forceinline__ void ob_pair(const RcObserveCall &c, float *X, float *Y, int lane) {
    float *io = POST ? Y : X;
    const RoLayer L = {io, RC_POLICY_DETER, nullptr, 0, XS, POST ? c.ws.obs2_w : c.wi.img3_w, POST ? c.ws.obs2_b : c.wi.img3_b,
                       RC_POLICY_LDPAIR, 32, io, RO_OUT, nullptr};
    ro_dense_pair(L, lane, [&](int row, int j, float mean, float raw) {
        io[row * XS + P_MEAN + j] = mean;
        io[row * XS + P_STD + j] = raw;
    });
}

// What follows a pair layer, one (row, column) per thread and pass: std = softplus(raw) + 0.1 where somebody reads it, the
// outputs, the KL's term (obs2; img3 leaves its std in place of the raw value for it) and stoch' where this layer gives it
template <bool SAMPLED, bool POST>
__device__ __forceinline__ void ob_pair_finish(const RcObserveCall &c, float *X, float *Y, float *Z, const float *normals, int64_t row0, int t, int tid) {
    const bool observed = t < c.context, gives_stoch = POST == observed;
    float *out_mean = POST ? c.post_mean : c.prior_mean, *out_std = POST ? c.post_std : c.prior_std;
    float *io = POST ? Y : X;
    const bool want_kl = c.kl != nullptr && observed;
    const bool want_std = out_std != nullptr || want_kl || (SAMPLED && gives_stoch);
#pragma unroll 1
    for (int idx = tid; idx < PM * RC_POLICY_STOCH; idx += PT) {
        const int row = idx / RC_POLICY_STOCH, j = idx - row * RC_POLICY_STOCH;
        const float mean = io[row * XS + P_MEAN + j];
        const float sd = want_std ? pm_softplus(io[row * XS + P_STD + j]) + PM_STOCH_MIN_STD : 0.0f;
        if (row0 + row < c.rows) {
            const size_t at = ((size_t)(row0 + row) * c.length + t) * RC_POLICY_STOCH + j;
            if (out_mean) out_mean[at] = mean;
            if (out_std) out_std[at] = sd;
        }
        if constexpr (POST) {
            if (want_kl) Y[row * XS + P_KL + j] = pm_kl_term(mean, sd, X[row * XS + P_MEAN + j], X[row * XS + P_STD + j]);
        } else if (want_kl) {
            X[row * XS + P_STD + j] = sd;
        }
        if (gives_stoch) {
            if constexpr (SAMPLED) Z[row * ZS + Z_STOCH + j] = fmaf(sd, normals[row * PN + j], mean);
            else Z[row * ZS + Z_STOCH + j] = mean;
        }
    }
}

template <bool SAMPLED>
__device__ __forceinline__ void ob_observe(const RcObserveCall &c) {
    extern __shared__ float ob_lds[];
    const RoLds lds = ro_carve(ob_lds);
    float *X = lds.X, *Y = lds.Y, *Z = lds.Z;
    float *normals = lds.rest;                               // [32][PN]   (sampled only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PM;
    const int T = c.length;

    // a row's window in the caller's arrays, -1 past the end
    auto window = [&](int row) { return row0 + row < c.rows ? row0 + row : (int64_t)-1; };
    // the start state: stoch | deter of state_in (its action columns are not read), or RSSM.initial's zeros; zero rows past the end
    ro_load_latent_rows(c.state_in, [&](int row) { return c.state_in ? window(row) : (int64_t)-1; }, Z, tid);
    __syncthreads();

    const bool head = c.reward != nullptr;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const bool observed = t < c.context;
        // (an observed step's prior is computed only where something of it is asked for: nothing else reads it)
        const bool need_prior = !observed || c.prior_mean || c.prior_std || c.kl;
        // the row's place in the caller's [rows][T] arrays at this step
        auto at_step = [&](int row) { return row0 + row < c.rows ? (row0 + row) * T + t : (int64_t)-1; };
        if constexpr (SAMPLED) {
            ro_stage_normals(normals, [&](int row) { return row0 + row < c.rows; }, [&](int row, uint32_t blk, float (&n)[4]) {
                const uint64_t id = c.row_offset + (uint64_t)(row0 + row);
                pm_observe_normal_block((uint32_t)id, (uint32_t)(id >> 32), (uint32_t)t, blk, c.seed_lo, c.seed_hi, n);
            }, false, tid);
        }
        ro_stage_actions(c.actions, nullptr, at_step, Z, tid);
        __syncthreads();
        // the head's one column
        auto out = [&](const RoLayer &L, int row, int, float v) {
            if (row0 + row < c.rows) L.g[(size_t)(row0 + row) * T + t] = v;
        };

        // ---- the prior step (img_step), then the head's three layers; the posterior sits between them (below)
        const int last = head ? 6 : 3;
#pragma unroll 1
        for (int layer = 0; layer < last; ++layer) {
            if (layer == 2) {
                if (need_prior) {
                    if (wave == 0) ob_pair<false>(c, X, Y, lane);
                    __syncthreads();
                    ob_pair_finish<SAMPLED, false>(c, X, Y, Z, normals, row0, t, tid);
                    __syncthreads();
                }
                if (observed) {
                    // ---- obs1 on [deter', embed]: deter' from Z, the scan in 9 pieces of 120 beams staged through X[0, 120)
                    // (clip / 15 - 0.5 applied on the way in), as rc_policy_kernel's; ELU -> Y[0, 200)
                    constexpr int PER = PM * SCK / PT;                       // 15 beams per thread and piece
                    float pre[PER];
                    auto request = [&](int piece) {
#pragma unroll
                        for (int i = 0; i < PER; ++i) {
                            const int idx = tid + PT * i, row = idx / SCK, b = idx - row * SCK;
                            pre[i] = row0 + row < c.rows ? c.scan[((size_t)(row0 + row) * T + t) * N_BEAMS + piece * SCK + b] : 0.0f;
                        }
                    };
                    request(0);
                    const int mine1 = (RC_POLICY_LD200 / 32 - wave + 3) / 4;      // 2, 2, 2, 1
                    int col[2] = {32 * wave, 32 * (wave + 4)};
                    if (mine1 < 2) col[1] = col[0];                                // (second tile unused: a valid column, never stored)
                    pm_f32x16 acc[2];
                    pm_bias<2>(acc, c.w.obs1_b, col, cc);
                    pm_gemm<2>(acc, Z + cc * ZS + half, RC_POLICY_DETER / 2, c.w.obs1_w + (size_t)half * RC_POLICY_LD200 + cc, RC_POLICY_LD200, col);
#pragma unroll 1
                    for (int piece = 0; piece < N_BEAMS / SCK; ++piece) {
                        __syncthreads();                                           // the readers of the previous piece are through
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
                    for (int i = 0; i < 2; ++i) {
                        const int j = col[i] + cc;
                        if (i >= mine1 || j >= RC_POLICY_DETER) continue;
#pragma unroll
                        for (int r = 0; r < 16; ++r) Y[pm_row(r, half) * XS + j] = pm_elu(acc[i][r]);
                    }
                    __syncthreads();
                    if (wave == 0) ob_pair<true>(c, X, Y, lane);
                    __syncthreads();
                    ob_pair_finish<SAMPLED, true>(c, X, Y, Z, normals, row0, t, tid);
                    __syncthreads();
                    // KL(post || prior) of the row: its 30 terms summed ascending
                    if (c.kl && tid < PM && row0 + tid < c.rows) {
                        float s = 0.0f;
                        for (int j = 0; j < RC_POLICY_STOCH; ++j) s = s + Y[tid * XS + P_KL + j];
                        c.kl[(size_t)(row0 + tid) * T + t] = s;
                    }
                }
                // feature[t] = [stoch', deter'] from the latent (its next writer is a barrier away); after the last step the state
                if (c.features) ro_store_features(c.features, at_step, Z, tid);
                if (c.state_out && t == T - 1) {
                    for (int idx = tid; idx < PM * RC_POLICY_STATE; idx += PT) {
                        const int row = idx / RC_POLICY_STATE, j = idx - row * RC_POLICY_STATE;
                        if (row0 + row < c.rows)
                            c.state_out[(size_t)(row0 + row) * RC_POLICY_STATE + j] =
                                Z[row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : (j < FEAT ? j - RC_POLICY_STOCH : j))];
                    }
                }
                continue;
            }
            RoLayer L;
            switch (layer) {
            case 0: L = ro_img1(Z, c.w, X); break;
            case 1: L = ro_img2(Y, c.wi, X); break;
            case 3: L = ro_first(Z, c.wi.rh_w[0], c.wi.rh_b[0], X); break;
            case 4: L = ro_hidden(X, c.wi.rh_w[1], c.wi.rh_b[1], Y); break;
            default: L = ro_column(Y, c.wi.rout_w, c.wi.rout_b, OK_REWARD, c.reward); break;
            }
            if (layer == 1) ro_commit_deter(Y, Z, tid);
            if (layer != 1 || need_prior) ro_layer(L, wave, lane, out);
            __syncthreads();
            if (layer != 0) continue;
            ro_gru(c.w, X, Z, Y, wave, lane);
            __syncthreads();
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_observe_kernel(RcObserveCall c) { ob_observe<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_observe_sampled_kernel(RcObserveCall c) { ob_observe<true>(c); }

hipError_t rck_observe_prepare() { return ro_prepare(rc_policy_observe_kernel, rc_policy_observe_sampled_kernel, kLdsBytes, kLdsBytesSampled); }

hipError_t rck_launch_observe(const RcObserveCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    return ro_launch(c.sample ? rc_policy_observe_sampled_kernel : rc_policy_observe_kernel, c.rows, c.sample ? kLdsBytesSampled : kLdsBytes,
                     c, start, stop, s);
}
