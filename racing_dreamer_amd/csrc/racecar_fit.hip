// rc_policy_fit_*: the reference's value update (dreamer/models.py:129-137: value_loss = -mean(weight * value(feat).log_prob(
// stop_gradient(returns))), value_opt on the value head's eight arrays alone; dreamer/tools.py:421-455 `Optimizer`: global-norm clip,
// then Adam) on the device, for the value head and - the same network with a Bernoulli output - the pcont head: one MLP's forward
// pass, backward pass, clip and Adam on tensors rc_policy_returns leaves on the device, in the binary32 arithmetic of DESIGN.md §2
// item 21 (tests/policy_fit_spec.c is the CPU restatement, one engine as here; the device equals it bit for bit).  Five launches on the handle's
// stream, no host round trip and no synchronisation in a step:
//   rc_policy_fit_rows_kernel   one workgroup of four waves per 32 rows, rc_policy_returns_kernel's geometry.  Forward through
//       the head, a1, a2, a3 kept (X, Y [32][417] in LDS and a global scratch [N][416] each); the output delta and the row's loss
//       term; then delta3 = (delta_o Wout^T) elu'(a3) in place of a3, delta2 = (delta3 W2^T) elu'(a2) in place of a2, delta1 =
//       (delta2 W1^T) elu'(a1) with a1 read back from the scratch its own lane wrote.  The transposed products read transposed
//       weight images [400][416] kept beside the forward images, so pm_gemm's B operand is coalesced as it is forward.  Each
//       product is a k-ascending fmaf chain from zero over the 400 units above (an MFMA chain: racecar_policy_tiles.h).
//   rc_policy_fit_wgrad_kernel  one workgroup per 32 x 32 tile of [a_{l-1} | 1]^T delta_l (the column of ones gives the bias
//       gradient: row K_l of the tile grid).  THE ORDER OF THE ROW SUM: row r belongs to chain (r / 2) mod 4 - wave w consumes the
//       row pairs w, w + 4, ..., one MFMA k-step each -, every chain is an fmaf chain from zero in ascending row order, and the
//       four are combined as (c0 + c1) + (c2 + c3) through LDS.  It depends on N alone: no atomics, nothing of the grid.
//       Padded rows and columns of the tiles are masked on the way in and never stored.
//   rc_policy_fit_sums_kernel   the sum of squares of the 413 601 gradient elements (array order, then element order) and the sum
//       of the N loss terms, both by one fixed tree in binary64: element i belongs to thread i mod 32 768 (128 workgroups of 256),
//       a thread adds its elements in ascending order, a workgroup halves its 256 sums seven times (t += t + stride, stride 128
//       .. 1), the 128 results are added in ascending order (rc_policy_fit_scale_kernel).
//   rc_policy_fit_scale_kernel  one thread: norm, loss, the clip scale, the skip of a step whose norm is not finite, the step
//       counter, the running powers of the betas and the bias-corrected rate.
//   rc_policy_fit_apply_kernel  g scale, Adam (TF's ResourceApplyAdam), the new weight into the forward image - the memory
//       rc_policy_returns and the rest read - and into the transposed image.
// The reward head (RC_POLICY_FIT_REWARD: the reference's DenseDecoder((), 2, 400) under the same Normal(o, 1); DESIGN.md §2 item 24,
// tests/policy_fit_spec.c at depth 2) is the same engine at two hidden layers: the rows kernel's body without the third layer and without
// the transposed product behind it (rc_policy_fit_reward_rows_kernel), the other four launches with a shorter table.  Its gradient is
// [231][400] | [401][400] | [401][1] = 253 201 elements, its scratch [4][N][416] + 2 N, its weights rc_policy_load_heads' images.
// The actor (RC_POLICY_FIT_ACTOR, rc_policy_actor_fit_step: the reference's ActionDecoder(2, 4, 400, 'tanh_normal'),
// dreamer/models.py:535-560, under actor_opt, dreamer/dream.py:87-88; DESIGN.md §2 item 25, tests/policy_actor_fit_spec.c's rule on that engine) is the
// engine at four hidden layers with a four-column output stage (rc_policy_fit_actor_rows_kernel): the output layer is read from the
// sampled modes' pair image [400][64] (mean columns 0, 1, raw std columns 32, 33), the tanh-normal action and its delta with respect
// to the four outputs take the place of the likelihood, the gradient with respect to the ACTIONS comes from the caller or from
// target actions, and the gradient with respect to the features, delta1 W0^T through a transposed image [400][256], is an output.
// Its gradient is [231][400] | 3 x [401][400] | [401][4] = 575 204 elements, its scratch [8][N][416] + 4 N + N; apply writes every
// image of the actor that a kernel reads: the hidden images, hout's mean image [400][32], the pair image, the transposed images.
// rc_policy_actor_forward_kernel is the same body's forward half alone: action, mean, std and nothing else.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

#include <cmath>

namespace {

constexpr int FS = 233;                        // row stride of the feature tile (odd: the 32 rows on 32 banks)
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER, UNITS = RC_POLICY_UNITS, LD = RC_POLICY_LD400;
constexpr int NOUT = 4;                        // the actor's output columns: mean 0, mean 1, raw std 0, raw std 1
constexpr size_t kFitLds = (size_t)(2 * PM * XS + PM * FS + PM * NOUT) * sizeof(float);
static_assert(kFitLds <= 160 * 1024, "X, Y, the feature tile and the output deltas [32][4]");
// the gradient, the moments: the head's eight arrays one behind the other, [K_l + 1][400] = kernel | bias per hidden layer, [401][1]
constexpr int G1 = (FEAT + 1) * UNITS, G2 = G1 + (UNITS + 1) * UNITS, GO = G2 + (UNITS + 1) * UNITS, NG = GO + UNITS + 1;
static_assert(NG == 413601, "230 x 400 + 400 + 2 (400 x 400 + 400) + 400 + 1");
// a head of `depth` hidden layers: where its output layer's [401][nout] lies in the gradient, and the gradient's length
constexpr int GL = (UNITS + 1) * UNITS;        // a hidden layer behind the first
__host__ __device__ constexpr int fit_go(int depth) { return G1 + (depth - 1) * GL; }
__host__ __device__ constexpr int fit_nout(int depth) { return depth == 4 ? NOUT : 1; }
__host__ __device__ constexpr int fit_ng(int depth) { return fit_go(depth) + (UNITS + 1) * fit_nout(depth); }
static_assert(fit_go(3) == GO && fit_go(2) == G2, "the layout of the value, pcont and reward heads' gradients");
static_assert(fit_ng(3) == NG && fit_ng(2) == 253201, "the value and pcont heads; the reward head");
static_assert(fit_ng(4) == 575204, "the actor: [231][400] | 3 x [401][400] | [401][4]");
constexpr int SUM_BLOCKS = 128, SUM_STRIDE = SUM_BLOCKS * PT;
constexpr float HALF_LOG_2PI = 0.9189385332f;

}  // namespace

struct FitCtl {                                // one per optimizer, on the device
    double part[2][SUM_BLOCKS];                // the workgroups' sums: squares of the gradient, loss terms
    double b1pow, b2pow;                       // beta^step, running products in binary64
    int32_t step, skipped;
    float scale, lr_t;
    float status[4];                           // loss, grad_norm, skipped, step
};

struct FitHeadDev {
    float *w[4], *b[4], *wout, *bout;          // the forward images (RcCriticDev's memory; the reward head: RcImagineDev's, two hidden
                                               // layers; the actor: RcPolicyDev's, four): [230 | 400][416], [416]; [400][32], [32]
    float *t[4];                               // t[l] = W_l^T [400][416], l = 1 .. depth - 1, padding zero; the actor alone: t[0] = W0^T
                                               // [400][256]
    float *wpair, *bpair;                      // the actor alone: hout's pair image [400][64], [64] (RcPolicySampleDev's), which the
                                               // rows kernel reads; wout, bout are then the mean image, which apply keeps equal
};

struct FitRowsCall {
    FitHeadDev h;
    const float *feat, *target, *weight;       // [N][230], [N] (the actor: target actions [N][2] or null), [N] or null
    int64_t n;
    float inv_n;
    int32_t pcont;
    float *act;                                // [6][N][416]: a1, a2, a3, delta1, delta2, delta3 (two hidden layers: [4][N][416]; four: [8][N][416])
    float *dout, *lterm;                       // [N] the output delta (the actor: [N][4]) and the loss term
    // the actor alone
    const float *eps, *grad;                   // [N][2] or null: the normal draw behind the action (null: the mode action); the gradient
                                               // with respect to the actions (exactly one of target and grad)
    float *gfeat;                              // [N][230] or null: the gradient with respect to the features
    float *o_action, *o_mean, *o_std;          // the forward-only kernel's outputs [N][2]; any may be null
};

namespace {

enum { FK_FORWARD = 0, FK_BACK_LDS = 1, FK_BACK_GLOBAL = 2 };

struct FitLayer {
    const float *a;                            // LDS input, rows `as` apart
    int k, as;
    const float *w, *b;                        // b null: the chain starts from zero
    float *d;                                  // LDS output [32][XS]; FK_BACK_LDS: holds the activation, overwritten; null: none
    const float *ga;                           // FK_BACK_GLOBAL: the activation's scratch
    float *g;                                  // the output's scratch [N][416]
    int kind;
};

__device__ __forceinline__ float fit_elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }

template <int TN, bool STORE>              // STORE false (the forward-only kernel): there is no scratch, L.g is not read
__device__ __forceinline__ void fit_dense(const FitLayer &L, int col0, int lane, int64_t row0, int64_t n) {
    const int cc = lane & 31, half = lane >> 5;
    int col[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) col[i] = col0 + 128 * i;
    pm_f32x16 acc[TN];
    if (L.b) {
        pm_bias<TN>(acc, L.b, col, cc);
    } else {
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    }
    pm_gemm<TN>(acc, L.a + cc * L.as + half, L.k / 2, L.w + (size_t)half * LD + cc, LD, col);
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int j = col[i] + cc;
        if (j >= UNITS) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = pm_row(r, half);
            const int64_t q = row0 + row;
            const bool valid = q < n;
            float v;
            if (L.kind == FK_FORWARD) {
                v = pm_elu(acc[i][r]);
            } else {
                const float a = L.kind == FK_BACK_LDS ? L.d[row * XS + j] : (valid ? L.ga[(size_t)q * LD + j] : 0.0f);
                v = acc[i][r] * fit_elu_grad(a);
            }
            if (L.d) L.d[row * XS + j] = v;
            if (STORE && valid) L.g[(size_t)q * LD + j] = v;
        }
    }
}

template <bool STORE = true>
__device__ __forceinline__ void fit_layer(const FitLayer &L, int wave, int lane, int64_t row0, int64_t n) {
    constexpr int n_tiles = LD / 32;
    const int mine = (n_tiles - wave + 3) / 4;          // tiles wave, wave + 4, ...: 4, 3, 3, 3
    if (mine == 4) fit_dense<4, STORE>(L, 32 * wave, lane, row0, n);
    else fit_dense<3, STORE>(L, 32 * wave, lane, row0, n);
}

// The gradient with respect to the features: delta1 (X, LDS) through W0^T [400][256], a k-ascending chain from zero over the 400
// units above; the 8 column tiles two per wave, the 26 padding columns (zero) never stored
__device__ __forceinline__ void fit_grad_features(const float *X, const float *t0, float *gfeat, int wave, int lane, int64_t row0, int64_t n) {
    const int cc = lane & 31, half = lane >> 5;
    const int col[2] = {32 * wave, 32 * (wave + 4)};
    pm_f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    pm_gemm<2>(acc, X + cc * XS + half, UNITS / 2, t0 + (size_t)half * RC_POLICY_LDT + cc, RC_POLICY_LDT, col);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = col[i] + cc;
        if (j >= FEAT) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t q = row0 + pm_row(r, half);
            if (q < n) gfeat[(size_t)q * FEAT + j] = acc[i][r];
        }
    }
}

// The rows kernel's body for a head of DEPTH hidden layers.  Two layers are three without the third layer's forward product and
// without the transposed product that takes delta3 to delta2: the last hidden activation is then in Y, not in X.  Four layers (the
// actor) ping-pong once more - a4 in Y, a3 still in X when the backward pass begins, a2 and a1 read back from the scratch their own
// lanes wrote - and have the four-column output stage.  FORWARD_ONLY (the actor): the forward pass and the action, no scratch.
template <int DEPTH, bool FORWARD_ONLY = false>
__device__ __forceinline__ void fit_rows(const FitRowsCall &c) {
    static_assert(DEPTH >= 2 && DEPTH <= 4 && (!FORWARD_ONLY || DEPTH == 4), "the reward head; the value and pcont heads; the actor");
    extern __shared__ float fit_lds[];
    float *X = fit_lds, *Y = fit_lds + PM * XS, *Z = fit_lds + 2 * PM * XS, *dl = Z + PM * FS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PM, n = c.n;
    const size_t plane = (size_t)n * LD;
    auto scratch = [&](int i) -> float * { return FORWARD_ONLY ? nullptr : c.act + (size_t)i * plane; };
    float *a1 = scratch(0), *a2 = scratch(1), *d1 = scratch(DEPTH), *d2 = scratch(DEPTH + 1);
    float *top = DEPTH == 3 ? X : Y, *dtop = scratch(2 * DEPTH - 1);                   // a_DEPTH's tile, delta_DEPTH's scratch

    for (int idx = tid; idx < PM * FS; idx += PT) {
        const int row = idx / FS, j = idx - row * FS;
        const int64_t q = row0 + row;
        Z[idx] = q < n && j < FEAT ? c.feat[(size_t)q * FEAT + j] : 0.0f;
    }
    __syncthreads();
    fit_layer<!FORWARD_ONLY>(FitLayer{Z, FEAT, FS, c.h.w[0], c.h.b[0], X, nullptr, a1, FK_FORWARD}, wave, lane, row0, n);
    __syncthreads();
    fit_layer<!FORWARD_ONLY>(FitLayer{X, UNITS, XS, c.h.w[1], c.h.b[1], Y, nullptr, a2, FK_FORWARD}, wave, lane, row0, n);
    __syncthreads();
    if constexpr (DEPTH >= 3) {
        fit_layer<!FORWARD_ONLY>(FitLayer{Y, UNITS, XS, c.h.w[2], c.h.b[2], X, nullptr, scratch(2), FK_FORWARD}, wave, lane, row0, n);
        __syncthreads();
    }
    if constexpr (DEPTH == 4) {
        fit_layer<!FORWARD_ONLY>(FitLayer{X, UNITS, XS, c.h.w[3], c.h.b[3], Y, nullptr, scratch(3), FK_FORWARD}, wave, lane, row0, n);
        __syncthreads();
    }
    if constexpr (DEPTH == 4) {
        // the four output columns, pm_dense_pair's scheme: lanes cc = 0, 1 of wave 0 hold the mean column cc in acc[0] and the raw
        // std column cc in acc[1], 16 rows each.  The tanh-normal action, then its delta with respect to the four outputs.  The
        // feature tile Z is free by now: Z[2 row + j] takes act_j - target_j for the loss term, which needs both j.
        if (wave == 0) {
            const int col[2] = {0, 32};
            pm_f32x16 acc[2];
            pm_bias<2>(acc, c.h.bpair, col, cc);
            pm_gemm<2>(acc, top + cc * XS + half, UNITS / 2, c.h.wpair + (size_t)half * RC_POLICY_LDPAIR + cc, RC_POLICY_LDPAIR, col);
            if (cc < 2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = pm_row(r, half);
                    const int64_t q = row0 + row;
                    float d_mean = 0.0f, d_std = 0.0f, diff = 0.0f;
                    if (q < n) {
                        const float th = pm_tanh(acc[0][r] / 5.0f);
                        const float mu = 5.0f * th;
                        const float raw = acc[1][r] + PM_RAW_INIT_STD;
                        const float sd = pm_softplus(raw) + PM_ACTION_MIN_STD;
                        const float e = c.eps ? c.eps[2 * (size_t)q + cc] : 0.0f;
                        const float u = c.eps ? fmaf(sd, e, mu) : mu;
                        const float a = pm_tanh(u);
                        if constexpr (FORWARD_ONLY) {
                            if (c.o_action) c.o_action[2 * (size_t)q + cc] = a;
                            if (c.o_mean) c.o_mean[2 * (size_t)q + cc] = mu;
                            if (c.o_std) c.o_std[2 * (size_t)q + cc] = sd;
                        } else {
                            float ga;
                            if (c.grad) {
                                ga = c.grad[2 * (size_t)q + cc];
                                if (c.weight) ga = c.weight[q] * ga;
                            } else {
                                diff = a - c.target[2 * (size_t)q + cc];
                                ga = diff;
                                if (c.weight) ga = c.weight[q] * ga;
                                ga = ga * c.inv_n;
                            }
                            const float du = ga * (1.0f - a * a);
                            d_mean = du * (1.0f - th * th);
                            if (c.eps) d_std = (du * e) * pm_sigmoid(raw);
                            c.dout[NOUT * (size_t)q + cc] = d_mean;
                            c.dout[NOUT * (size_t)q + 2 + cc] = d_std;
                        }
                    }
                    if constexpr (!FORWARD_ONLY) {
                        dl[NOUT * row + cc] = d_mean;
                        dl[NOUT * row + 2 + cc] = d_std;
                        Z[2 * row + cc] = diff;
                    }
                }
            }
        }
        if constexpr (FORWARD_ONLY) return;
        __syncthreads();
        // the row's loss term, negated (rc_policy_fit_scale_kernel takes minus the mean): -(w (0.5 (d0 d0 + d1 d1))); grad mode: +0
        if (tid < PM && row0 + tid < n) {
            float l = 0.0f;
            if (!c.grad) {
                l = 0.5f * fmaf(Z[2 * tid + 1], Z[2 * tid + 1], Z[2 * tid] * Z[2 * tid]);
                if (c.weight) l = c.weight[row0 + tid] * l;
                l = -l;
            }
            c.lterm[row0 + tid] = l;
        }
        // delta4 in place of a4: a chain of four products from zero, the output columns in ascending order
        for (int idx = tid; idx < PM * UNITS; idx += PT) {
            const int row = idx / UNITS, j = idx - row * UNITS;
            const int64_t q = row0 + row;
            const float *wr = c.h.wpair + (size_t)j * RC_POLICY_LDPAIR;
            float s = fmaf(dl[NOUT * row], wr[0], 0.0f);
            s = fmaf(dl[NOUT * row + 1], wr[1], s);
            s = fmaf(dl[NOUT * row + 2], wr[32], s);
            s = fmaf(dl[NOUT * row + 3], wr[33], s);
            const float v = s * fit_elu_grad(top[row * XS + j]);
            top[row * XS + j] = v;
            if (q < n) dtop[(size_t)q * LD + j] = v;
        }
        __syncthreads();
        fit_layer(FitLayer{Y, UNITS, XS, c.h.t[3], nullptr, X, nullptr, scratch(DEPTH + 2), FK_BACK_LDS}, wave, lane, row0, n);
        __syncthreads();
        fit_layer(FitLayer{X, UNITS, XS, c.h.t[2], nullptr, Y, a2, d2, FK_BACK_GLOBAL}, wave, lane, row0, n);
        __syncthreads();
        fit_layer(FitLayer{Y, UNITS, XS, c.h.t[1], nullptr, c.gfeat ? X : nullptr, a1, d1, FK_BACK_GLOBAL}, wave, lane, row0, n);
        if (c.gfeat) {
            __syncthreads();
            fit_grad_features(X, c.h.t[0], c.gfeat, wave, lane, row0, n);
        }
    } else {
        // the one output column: lanes 0 and 32 of wave 0 hold it for 16 rows each; the output delta and the row's loss term
        if (wave == 0) {
            const int col[1] = {0};
            pm_f32x16 acc[1];
            pm_bias<1>(acc, c.h.bout, col, cc);
            pm_gemm<1>(acc, top + cc * XS + half, UNITS / 2, c.h.wout + (size_t)half * RC_POLICY_LDSMALL + cc, RC_POLICY_LDSMALL, col);
            if (cc == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = pm_row(r, half);
                    const int64_t q = row0 + row;
                    float delta = 0.0f;
                    if (q < n) {
                        const float o = acc[0][r], t = c.target[q];
                        float e, lp;
                        if (c.pcont) {
                            lp = -fmaf(t, pm_softplus(-o), (1.0f - t) * pm_softplus(o));
                            e = pm_sigmoid(o) - t;
                        } else {
                            e = o - t;
                            lp = fmaf(-0.5f, e * e, -HALF_LOG_2PI);
                        }
                        if (c.weight) {
                            const float w = c.weight[q];
                            e = w * e;
                            lp = w * lp;
                        }
                        delta = e * c.inv_n;
                        c.dout[q] = delta;
                        c.lterm[q] = lp;
                    }
                    dl[row] = delta;
                }
            }
        }
        __syncthreads();
        // delta3 in place of a3 (two layers: delta2 in place of a2): a chain of one product from zero
        for (int idx = tid; idx < PM * UNITS; idx += PT) {
            const int row = idx / UNITS, j = idx - row * UNITS;
            const int64_t q = row0 + row;
            const float v = fmaf(dl[row], c.h.wout[(size_t)j * RC_POLICY_LDSMALL], 0.0f) * fit_elu_grad(top[row * XS + j]);
            top[row * XS + j] = v;
            if (q < n) dtop[(size_t)q * LD + j] = v;
        }
        __syncthreads();
        if constexpr (DEPTH == 3) {
            fit_layer(FitLayer{X, UNITS, XS, c.h.t[2], nullptr, Y, nullptr, d2, FK_BACK_LDS}, wave, lane, row0, n);
            __syncthreads();
        }
        fit_layer(FitLayer{Y, UNITS, XS, c.h.t[1], nullptr, nullptr, a1, d1, FK_BACK_GLOBAL}, wave, lane, row0, n);
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_fit_rows_kernel(FitRowsCall c) { fit_rows<3>(c); }
__global__ __launch_bounds__(PT) void rc_policy_fit_reward_rows_kernel(FitRowsCall c) { fit_rows<2>(c); }
__global__ __launch_bounds__(PT) void rc_policy_fit_actor_rows_kernel(FitRowsCall c) { fit_rows<4>(c); }
__global__ __launch_bounds__(PT) void rc_policy_actor_forward_kernel(FitRowsCall c) { fit_rows<4, true>(c); }

struct FitWgradCall {
    const float *a[5];                         // a_{l-1} [N][lda]: the features, a1, a2, a3 (the actor: a4)
    const float *d[5];                         // delta_l [N][ldd]: delta1, delta2, delta3 (the actor: delta4), the output delta
    int32_t lda[5], ldd[5], k[5], nc[5];       // K_l = 230, 400, 400, 400 (, 400); the columns 400, 400, 400 (, 400), 1 (the actor: 4)
    int32_t tile0[5], nt[5], goff[5];          // the layer's first workgroup, its column tiles, its place in the gradient
                                               // (depth + 1 entries; the others' tile0 is the grid, no workgroup is theirs)
    float *g;                                  // [fit_ng(depth)]
    int64_t n;
};

namespace {

constexpr int WU = 16;                         // row pairs whose operands a wave requests one block ahead

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_fit_wgrad_kernel(FitWgradCall c) {
    __shared__ float red[4][32][33];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int b = blockIdx.x;
    const int l = b >= c.tile0[4] ? 4 : (b >= c.tile0[3] ? 3 : (b >= c.tile0[2] ? 2 : (b >= c.tile0[1] ? 1 : 0)));
    const int t = b - c.tile0[l], kt = t / c.nt[l], jt = t - kt * c.nt[l];
    const int K = c.k[l], NC = c.nc[l], lda = c.lda[l], ldd = c.ldd[l];
    const int kcol = 32 * kt + cc, ncol = 32 * jt + cc;
    const bool a_mem = kcol < K, a_one = kcol == K, d_mem = ncol < NC;
    const float *A = c.a[l] + (a_mem ? kcol : 0), *D = c.d[l] + (d_mem ? ncol : 0);
    const int64_t n = c.n, pairs = (n + 1) / 2;
    pm_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    // a row past the end, a padded column: both operands zero, and fmaf(0, 0, acc) = acc (acc is never -0: it starts at +0)
    // the operands of the next WU pairs are requested before this block's MFMAs issue (pm_gemm's scheme): a wave's chain is
    // serial, so the loads' latency has to hide behind the MFMAs of the block before
    float ac[WU], dc[WU], an[WU], dn[WU];
    auto request = [&](int64_t s0, float (&av)[WU], float (&dv)[WU]) {
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            const int64_t r = 2 * (s0 + 4 * u) + half;
            const bool in = r < n;
            av[u] = in ? (a_mem ? A[(size_t)r * lda] : (a_one ? 1.0f : 0.0f)) : 0.0f;
            dv[u] = in && d_mem ? D[(size_t)r * ldd] : 0.0f;
        }
    };
    request(wave, ac, dc);
#pragma unroll 1
    for (int64_t s0 = wave; s0 < pairs; s0 += 4 * WU) {
        request(s0 + 4 * WU, an, dn);
#pragma unroll
        for (int u = 0; u < WU; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u], dc[u], acc, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            ac[u] = an[u];
            dc[u] = dn[u];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][pm_row(r, half)][cc] = acc[r];
    __syncthreads();
    for (int idx = tid; idx < 32 * 32; idx += PT) {
        const int i = idx >> 5, j = idx & 31;
        const int kk = 32 * kt + i, jj = 32 * jt + j;
        const float v = (red[0][i][j] + red[1][i][j]) + (red[2][i][j] + red[3][i][j]);
        if (kk <= K && jj < NC) c.g[(size_t)c.goff[l] + (size_t)kk * NC + jj] = v;
    }
}

__global__ __launch_bounds__(PT) void rc_policy_fit_sums_kernel(const float *g, int ng, const float *lterm, int64_t n, FitCtl *ctl) {
    __shared__ double sh[PT];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int which = 0; which < 2; ++which) {
        const int64_t count = which == 0 ? (int64_t)ng : n;
        double s = 0.0;
        for (int64_t i = (int64_t)b * PT + tid; i < count; i += SUM_STRIDE) {
            const float x = which == 0 ? g[i] : lterm[i];
            const float q = which == 0 ? x * x : x;
            s += (double)q;
        }
        sh[tid] = s;
        __syncthreads();
        for (int stride = PT / 2; stride >= 1; stride >>= 1) {
            if (tid < stride) sh[tid] += sh[tid + stride];
            __syncthreads();
        }
        if (tid == 0) ctl->part[which][b] = sh[0];
        __syncthreads();
    }
}

__global__ void rc_policy_fit_scale_kernel(FitCtl *ctl, int64_t n, float lr, float clip, float beta1, float beta2, float *status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sq = 0.0, ls = 0.0;
    for (int b = 0; b < SUM_BLOCKS; ++b) sq += ctl->part[0][b];
    for (int b = 0; b < SUM_BLOCKS; ++b) ls += ctl->part[1][b];
    const float norm = (float)sqrt(sq);
    const float loss = (float)(-(ls / (double)n));
    const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
    if (finite) {
        ctl->step += 1;
        ctl->b1pow = ctl->b1pow * (double)beta1;
        ctl->b2pow = ctl->b2pow * (double)beta2;
        const float c1 = (float)(1.0 - ctl->b1pow), c2 = (float)(1.0 - ctl->b2pow);
        ctl->lr_t = (lr * (float)sqrt((double)c2)) / c1;
        ctl->scale = clip > 0.0f ? clip / (norm > clip ? norm : clip) : 1.0f;
    }
    ctl->skipped = finite ? 0 : 1;
    ctl->status[0] = loss;
    ctl->status[1] = norm;
    ctl->status[2] = finite ? 0.0f : 1.0f;
    ctl->status[3] = (float)ctl->step;
    if (status)
        for (int i = 0; i < 4; ++i) status[i] = ctl->status[i];
}

__global__ __launch_bounds__(PT) void rc_policy_fit_apply_kernel(FitHeadDev h, int depth, const float *g, float *m, float *v, const FitCtl *ctl,
                                                                 float beta1, float beta2, float omb1, float omb2, float epsilon) {
    const int e = blockIdx.x * PT + threadIdx.x;
    const int go = fit_go(depth), nout = fit_nout(depth);
    if (e >= go + (UNITS + 1) * nout || ctl->skipped) return;
    float *w, *wt = nullptr;                   // the weight, and its second image: the transposed one, or hout's mean image (the actor)
    if (e < go) {
        const int l = e < G1 ? 0 : 1 + (e - G1) / GL;
        const int i = e - (l == 0 ? 0 : G1 + (l - 1) * GL), K = l == 0 ? FEAT : UNITS;
        const int k = i / UNITS, j = i - k * UNITS;
        w = k < K ? h.w[l] + (size_t)k * LD + j : h.b[l] + j;
        if (k < K && h.t[l]) wt = h.t[l] + (size_t)j * (l == 0 ? RC_POLICY_LDT : LD) + k;
    } else if (nout == 1) {
        const int k = e - go;
        w = k < UNITS ? h.wout + (size_t)k * RC_POLICY_LDSMALL : h.bout;
    } else {                                   // the actor's [401][4]: column c is the pair image's column c (mean) or 32 + c - 2 (raw std)
        const int k = (e - go) / NOUT, c = (e - go) - k * NOUT;
        const int pc = c < 2 ? c : 32 + c - 2;
        w = k < UNITS ? h.wpair + (size_t)k * RC_POLICY_LDPAIR + pc : h.bpair + pc;
        if (c < 2) wt = k < UNITS ? h.wout + (size_t)k * RC_POLICY_LDSMALL + c : h.bout + c;
    }
    const float gs = g[e] * ctl->scale;
    const float mn = fmaf(beta1, m[e], omb1 * gs);
    const float vn = fmaf(beta2, v[e], omb2 * (gs * gs));
    const float den = (float)sqrt((double)vn) + epsilon;      // (the binary64 root rounds to the correctly rounded binary32 one)
    const float wn = fmaf(-ctl->lr_t, mn / den, *w);
    m[e] = mn;
    v[e] = vn;
    *w = wn;
    if (wt) *wt = wn;
}

// W [k_in][416] -> W^T [400][ldt], the padding columns zero ([400][416] -> [400][416]; the actor's W0 [230][416] -> [400][256])
__global__ __launch_bounds__(PT) void rc_policy_fit_transpose_kernel(const float *w, float *t, int k_in, int ldt) {
    const int idx = blockIdx.x * PT + threadIdx.x;
    if (idx >= UNITS * ldt) return;
    const int j = idx / ldt, k = idx - j * ldt;
    t[idx] = k < k_in ? w[(size_t)k * LD + j] : 0.0f;
}

// ---- the optimizers of a handle and the entry points (include/racecar_hip.h, rc_policy_fit_*, rc_policy_actor_*)
constexpr int kFitHeads = 4;                   // RC_POLICY_FIT_VALUE, _PCONT, _REWARD, _ACTOR

struct RcFit {
    struct Head {
        float *mem = nullptr;                  // m [ng] | v [ng] | g [ng] | W1^T | W2^T (the reward head: W1^T alone; the actor: W1^T | W2^T | W3^T | W0^T)
        FitCtl *ctl = nullptr;
    } head[kFitHeads];
    float *scratch = nullptr;                  // [2 depth][rows][416] | the output delta [rows][nout] | the loss terms [rows]: the heads share it
    size_t scratch_floats = 0;
};

namespace {

constexpr size_t kImage = (size_t)UNITS * LD;
constexpr size_t kImage0 = (size_t)UNITS * RC_POLICY_LDT;      // the actor's W0^T

constexpr int fit_depth(int head) { return head == RC_POLICY_FIT_ACTOR ? 4 : (head == RC_POLICY_FIT_REWARD ? 2 : 3); }
constexpr size_t fit_moment(int depth) { return ((size_t)fit_ng(depth) + 63) / 64 * 64; }

FitHeadDev fit_head(rc_env *env, int head) {
    const RcCriticDev &c = env->pol_c;
    const RcImagineDev &r = env->pol_i;
    FitHeadDev h{};
    if (head == RC_POLICY_FIT_ACTOR) {
        for (int l = 0; l < 4; ++l) {
            h.w[l] = const_cast<float *>(env->pol.h_w[l]);
            h.b[l] = const_cast<float *>(env->pol.h_b[l]);
        }
        h.wout = const_cast<float *>(env->pol.hout_w);
        h.bout = const_cast<float *>(env->pol.hout_b);
        h.wpair = const_cast<float *>(env->pol_s.hout_w);
        h.bpair = const_cast<float *>(env->pol_s.hout_b);
    } else if (head == RC_POLICY_FIT_REWARD) {
        for (int l = 0; l < 2; ++l) {
            h.w[l] = const_cast<float *>(r.rh_w[l]);
            h.b[l] = const_cast<float *>(r.rh_b[l]);
        }
        h.wout = const_cast<float *>(r.rout_w);
        h.bout = const_cast<float *>(r.rout_b);
    } else {
        for (int l = 0; l < 3; ++l) {
            h.w[l] = const_cast<float *>(head ? c.ph_w[l] : c.vh_w[l]);
            h.b[l] = const_cast<float *>(head ? c.ph_b[l] : c.vh_b[l]);
        }
        h.wout = const_cast<float *>(head ? c.pout_w : c.vout_w);
        h.bout = const_cast<float *>(head ? c.pout_b : c.vout_b);
    }
    if (env->fit && env->fit->head[head].mem) {
        const int depth = fit_depth(head);
        float *t = env->fit->head[head].mem + 3 * fit_moment(depth);
        for (int l = 1; l < depth; ++l) h.t[l] = t + (size_t)(l - 1) * kImage;
        if (depth == 4) h.t[0] = t + 3 * kImage;
    }
    return h;
}

int fit_close(rc_env *env, int head) {
    if (!env->fit || !env->fit->head[head].mem) return RC_OK;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    RcFit::Head &o = env->fit->head[head];
    (void)hipFree(o.mem);
    (void)hipFree(o.ctl);
    o = RcFit::Head{};
    bool any = false;
    for (const RcFit::Head &other : env->fit->head) any = any || other.mem;
    if (!any) {
        if (env->fit->scratch) (void)hipFree(env->fit->scratch);
        delete env->fit;
        env->fit = nullptr;
    }
    return RC_OK;
}

const char *fit_head_name(int head) {
    return head == RC_POLICY_FIT_ACTOR ? "actor" : (head == RC_POLICY_FIT_REWARD ? "reward" : (head == RC_POLICY_FIT_PCONT ? "pcont" : "value"));
}
bool fit_head_known(int head) {
    return head == RC_POLICY_FIT_VALUE || head == RC_POLICY_FIT_PCONT || head == RC_POLICY_FIT_REWARD || head == RC_POLICY_FIT_ACTOR;
}

hipError_t fit_prepare() {
    const void *rows[] = {(const void *)rc_policy_fit_rows_kernel, (const void *)rc_policy_fit_reward_rows_kernel,
                          (const void *)rc_policy_fit_actor_rows_kernel, (const void *)rc_policy_actor_forward_kernel};
    for (const void *k : rows) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitLds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the actor that the engine fits is loaded and plain: `fn` words the refusal
int fit_actor_check(rc_env *env, const char *fn) {
    if (!env->pol_mem || !env->pol.hout_w) return fail(RC_ERR_INVALID, "%s: no policy loaded (rc_policy_load)", fn);
    if (env->pol.hnorm)
        return fail(RC_ERR_INVALID, "%s: the loaded actor is normalized (hnorm_*: batch statistics in training), the engine fits the plain actor alone", fn);
    return RC_OK;
}

struct FitHyper { float lr, clip, beta1, beta2, epsilon; };

int fit_check_step(const char *fn, int64_t rows, const FitHyper &hp) {
    if (rows < 1 || rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "%s: rows %lld is outside [1, 2^31)", fn, (long long)rows);
    const float hyper[5] = {hp.lr, hp.clip, hp.beta1, hp.beta2, hp.epsilon};
    const char *names[5] = {"lr", "clip", "beta1", "beta2", "epsilon"};
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(hyper[i]) || hyper[i] < 0.0f)
            return fail(RC_ERR_INVALID, "%s: %s %g is not a finite number >= 0", fn, names[i], (double)hyper[i]);
    if (hp.beta1 >= 1.0f || hp.beta2 >= 1.0f)
        return fail(RC_ERR_INVALID, "%s: beta1 %g, beta2 %g: both must lie in [0, 1)", fn, (double)hp.beta1, (double)hp.beta2);
    return RC_OK;
}

// One step of an open optimizer: the five launches.  `r` carries the caller's tensors (feat, target, weight; the actor: eps, grad,
// gfeat); the checks are the caller's.
int fit_run(rc_env *env, int head, int64_t n, FitRowsCall r, const FitHyper &hp, float *status) {
    const int depth = fit_depth(head), ng = fit_ng(depth), nout = fit_nout(depth);
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcFit &f = *env->fit;
    const size_t need = (size_t)n * (2 * depth * LD + nout + 1);
    if (need > f.scratch_floats) {
        if (f.scratch) {
            HIP_TRY(hipStreamSynchronize(env->stream));
            (void)hipFree(f.scratch);
            f.scratch = nullptr;
            f.scratch_floats = 0;
        }
        HIP_TRY(hipMalloc((void **)&f.scratch, need * sizeof(float)));
        f.scratch_floats = need;
    }
    RcFit::Head &o = f.head[head];
    const size_t kMoment = fit_moment(depth);
    float *m = o.mem, *v = o.mem + kMoment, *g = o.mem + 2 * kMoment;
    const size_t plane = (size_t)n * LD;
    r.h = fit_head(env, head);
    r.n = n;
    r.inv_n = 1.0f / (float)n;
    r.pcont = head == RC_POLICY_FIT_PCONT;
    r.act = f.scratch;
    r.dout = f.scratch + 2 * depth * plane;
    r.lterm = r.dout + (size_t)n * nout;
    FitWgradCall w{};
    int tiles = 0;
    for (int l = 0; l <= depth; ++l) {          // layer l's input a_l (the features, a1 ..) and delta_{l+1} (.., the output delta)
        const bool out = l == depth;
        w.a[l] = l == 0 ? r.feat : r.act + (size_t)(l - 1) * plane;
        w.d[l] = out ? r.dout : r.act + (size_t)(depth + l) * plane;
        w.lda[l] = l == 0 ? FEAT : LD;
        w.ldd[l] = out ? nout : LD;
        w.k[l] = l == 0 ? FEAT : UNITS;
        w.nc[l] = out ? nout : UNITS;
        w.tile0[l] = tiles;
        w.nt[l] = (w.nc[l] + 31) / 32;
        w.goff[l] = l == 0 ? 0 : G1 + (l - 1) * GL;
        tiles += (w.k[l] + 1 + 31) / 32 * w.nt[l];
    }
    for (int l = depth + 1; l < 5; ++l) w.tile0[l] = tiles;
    w.g = g;
    w.n = n;
    KernelTimer t;
    int rc = t.begin(env, RC_K_POLICY, true);
    if (rc) return rc;
    const dim3 row_blocks((unsigned)((n + PM - 1) / PM));
    if (depth == 4) hipLaunchKernelGGL(rc_policy_fit_actor_rows_kernel, row_blocks, dim3(PT), (uint32_t)kFitLds, env->stream, r);
    else if (depth == 3) hipLaunchKernelGGL(rc_policy_fit_rows_kernel, row_blocks, dim3(PT), (uint32_t)kFitLds, env->stream, r);
    else hipLaunchKernelGGL(rc_policy_fit_reward_rows_kernel, row_blocks, dim3(PT), (uint32_t)kFitLds, env->stream, r);
    hipLaunchKernelGGL(rc_policy_fit_wgrad_kernel, dim3((unsigned)tiles), dim3(PT), 0, env->stream, w);
    hipLaunchKernelGGL(rc_policy_fit_sums_kernel, dim3(SUM_BLOCKS), dim3(PT), 0, env->stream, (const float *)g, ng, (const float *)r.lterm, n, o.ctl);
    hipLaunchKernelGGL(rc_policy_fit_scale_kernel, dim3(1), dim3(64), 0, env->stream, o.ctl, n, hp.lr, hp.clip, hp.beta1, hp.beta2, status);
    hipLaunchKernelGGL(rc_policy_fit_apply_kernel, dim3((ng + PT - 1) / PT), dim3(PT), 0, env->stream, r.h, depth, (const float *)g, m, v,
                       (const FitCtl *)o.ctl, hp.beta1, hp.beta2, 1.0f - hp.beta1, 1.0f - hp.beta2, hp.epsilon);
    // rc_policy_dream_grad keeps transposed copies of the reward head's two hidden layers: its next call makes them again, on the stream
    if (head == RC_POLICY_FIT_REWARD) env->dgrad_reward_stale = true;
    // rc_policy_returns_grad keeps such copies of every head it carries a cotangent through (not of the actor)
    env->rgrad_stale |= head == RC_POLICY_FIT_REWARD ? RC_RGRAD_REWARD : (head == RC_POLICY_FIT_VALUE ? RC_RGRAD_VALUE : (head == RC_POLICY_FIT_PCONT ? RC_RGRAD_PCONT : 0u));
    HIP_TRY(hipGetLastError());
    return t.end();
}

}  // namespace

// rc_policy_load_critic, rc_policy_load, rc_policy_unload and rc_destroy close the critic's optimizers
int fit_release(rc_env *env) {
    const int rc = fit_close(env, RC_POLICY_FIT_VALUE);
    return rc ? rc : fit_close(env, RC_POLICY_FIT_PCONT);
}

// rc_policy_load_heads, rc_policy_load, rc_policy_unload and rc_destroy close the reward head's
int fit_release_reward(rc_env *env) { return fit_close(env, RC_POLICY_FIT_REWARD); }

// rc_policy_load_actor, rc_policy_load, rc_policy_unload and rc_destroy close the actor's
int fit_release_actor(rc_env *env) { return fit_close(env, RC_POLICY_FIT_ACTOR); }

extern "C" {

int rc_policy_fit_begin(rc_env *env, const rc_policy_fit_config *cfg) {
    if (!env || !cfg) return fail(RC_ERR_INVALID, "NULL argument");
    if (cfg->struct_size != sizeof(rc_policy_fit_config))
        return fail(RC_ERR_INVALID, "rc_policy_fit_config.struct_size %u != %zu", cfg->struct_size, sizeof(rc_policy_fit_config));
    if (!fit_head_known(cfg->head)) return fail(RC_ERR_INVALID, "rc_policy_fit_begin: unknown head %d", cfg->head);
    const int head = cfg->head, depth = fit_depth(head);
    if (head == RC_POLICY_FIT_ACTOR) {
        const int rc_actor = fit_actor_check(env, "rc_policy_fit_begin");
        if (rc_actor) return rc_actor;
    } else if (!fit_head(env, head).wout) {
        return fail(RC_ERR_INVALID, "rc_policy_fit_begin: no %s head is loaded (%s)", fit_head_name(head),
                    head == RC_POLICY_FIT_REWARD ? "rc_policy_load_heads" : "rc_policy_load_critic");
    }
    int rc = fit_close(env, head);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(fit_prepare());
    if (!env->fit) env->fit = new RcFit();
    RcFit::Head &o = env->fit->head[head];
    const size_t kMoment = fit_moment(depth), floats = 3 * kMoment + (size_t)(depth - 1) * kImage + (depth == 4 ? kImage0 : 0);
    hipError_t e = hipMalloc((void **)&o.mem, floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&o.ctl, sizeof(FitCtl));
    if (e != hipSuccess) {
        if (o.mem) (void)hipFree(o.mem);
        o = RcFit::Head{};
        return fail(RC_ERR_HIP, "rc_policy_fit_begin: %s", hipGetErrorString(e));
    }
    HIP_TRY(hipMemsetAsync(o.mem, 0, 3 * kMoment * sizeof(float), env->stream));
    FitCtl init{};
    init.b1pow = init.b2pow = 1.0;
    init.scale = 1.0f;
    HIP_TRY(hipMemcpyAsync(o.ctl, &init, sizeof init, hipMemcpyHostToDevice, env->stream));
    const FitHeadDev h = fit_head(env, head);
    const unsigned blocks = (unsigned)((kImage + PT - 1) / PT);
    for (int l = 1; l < depth; ++l)
        hipLaunchKernelGGL(rc_policy_fit_transpose_kernel, dim3(blocks), dim3(PT), 0, env->stream, (const float *)h.w[l], h.t[l], UNITS, LD);
    if (depth == 4)
        hipLaunchKernelGGL(rc_policy_fit_transpose_kernel, dim3((unsigned)((kImage0 + PT - 1) / PT)), dim3(PT), 0, env->stream, (const float *)h.w[0],
                           h.t[0], FEAT, RC_POLICY_LDT);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(env->stream));             // (`init` goes out of scope)
    return RC_OK;
}

int rc_policy_fit_step(rc_env *env, const rc_policy_fit_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_fit_args))
        return fail(RC_ERR_INVALID, "rc_policy_fit_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_fit_args));
    if (!fit_head_known(a->head)) return fail(RC_ERR_INVALID, "rc_policy_fit_step: unknown head %d", a->head);
    const int head = a->head;
    if (head == RC_POLICY_FIT_ACTOR) return fail(RC_ERR_INVALID, "rc_policy_fit_step: the actor's step is rc_policy_actor_fit_step");
    if (!env->fit || !env->fit->head[head].mem)
        return fail(RC_ERR_INVALID, "rc_policy_fit_step: no optimizer is open for the %s head (rc_policy_fit_begin)", fit_head_name(head));
    if (!a->features || !a->target) return fail(RC_ERR_INVALID, "rc_policy_fit_step: %s is NULL", !a->features ? "features" : "target");
    const FitHyper hp{a->lr, a->clip, a->beta1, a->beta2, a->epsilon};
    const int rc = fit_check_step("rc_policy_fit_step", a->rows, hp);
    if (rc) return rc;
    FitRowsCall r{};
    r.feat = a->features; r.target = a->target; r.weight = a->weight;
    return fit_run(env, head, a->rows, r, hp, a->status);
}

int rc_policy_fit_end(rc_env *env, int32_t head) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!fit_head_known(head)) return fail(RC_ERR_INVALID, "rc_policy_fit_end: unknown head %d", head);
    return fit_close(env, head);
}

int rc_policy_actor_fit_step(rc_env *env, const rc_policy_actor_fit_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_actor_fit_args))
        return fail(RC_ERR_INVALID, "rc_policy_actor_fit_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_actor_fit_args));
    int rc = fit_actor_check(env, "rc_policy_actor_fit_step");
    if (rc) return rc;
    if (!env->fit || !env->fit->head[RC_POLICY_FIT_ACTOR].mem)
        return fail(RC_ERR_INVALID, "rc_policy_actor_fit_step: no optimizer is open for the actor (rc_policy_fit_begin with RC_POLICY_FIT_ACTOR)");
    if (!a->features) return fail(RC_ERR_INVALID, "rc_policy_actor_fit_step: features is NULL");
    if (!a->target == !a->grad)
        return fail(RC_ERR_INVALID, "rc_policy_actor_fit_step: %s of target and grad given (exactly one)", a->target ? "both" : "neither");
    const FitHyper hp{a->lr, a->clip, a->beta1, a->beta2, a->epsilon};
    rc = fit_check_step("rc_policy_actor_fit_step", a->rows, hp);
    if (rc) return rc;
    FitRowsCall r{};
    r.feat = a->features; r.target = a->target; r.weight = a->weight;
    r.eps = a->eps; r.grad = a->grad; r.gfeat = a->grad_features;
    return fit_run(env, RC_POLICY_FIT_ACTOR, a->rows, r, hp, a->status);
}

int rc_policy_actor_forward(rc_env *env, const rc_policy_actor_forward_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_actor_forward_args))
        return fail(RC_ERR_INVALID, "rc_policy_actor_forward_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_actor_forward_args));
    const int rc = fit_actor_check(env, "rc_policy_actor_forward");
    if (rc) return rc;
    if (!a->features) return fail(RC_ERR_INVALID, "rc_policy_actor_forward: features is NULL");
    if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_actor_forward: rows %lld is outside [1, 2^31)", (long long)a->rows);
    if (!a->action && !a->mean && !a->std) return fail(RC_ERR_INVALID, "rc_policy_actor_forward: no output asked for");
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(fit_prepare());
    FitRowsCall r{};
    r.h = fit_head(env, RC_POLICY_FIT_ACTOR);
    r.feat = a->features; r.eps = a->eps;
    r.n = a->rows;
    r.o_action = a->action; r.o_mean = a->mean; r.o_std = a->std;
    KernelTimer t;
    const int rc_t = t.begin(env, RC_K_POLICY, true);
    if (rc_t) return rc_t;
    hipLaunchKernelGGL(rc_policy_actor_forward_kernel, dim3((unsigned)((a->rows + PM - 1) / PM)), dim3(PT), (uint32_t)kFitLds, env->stream, r);
    HIP_TRY(hipGetLastError());
    return t.end();
}

}  // extern "C"
