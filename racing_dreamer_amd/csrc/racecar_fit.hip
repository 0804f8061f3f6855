// rc_policy_fit_*: the reference's value update (dreamer/models.py:129-137: value_loss = -mean(weight * value(feat).log_prob(
// stop_gradient(returns))), value_opt on the value head's eight arrays alone; dreamer/tools.py:421-455 `Optimizer`: global-norm clip,
// then Adam) on the device, for the value head and - the same network with a Bernoulli output - the pcont head: one MLP's forward
// pass, backward pass, clip and Adam on tensors rc_policy_returns leaves on the device, in the binary32 arithmetic of DESIGN.md §2
// item 21 (tests/policy_fit_spec.c is the CPU restatement; the device equals it bit for bit).  Five launches on the handle's
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
// tests/policy_reward_fit_spec.c) is the same engine at two hidden layers: the rows kernel's body without the third layer and without
// the transposed product behind it (rc_policy_fit_reward_rows_kernel), the other four launches with a shorter table.  Its gradient is
// [231][400] | [401][400] | [401][1] = 253 201 elements, its scratch [4][N][416] + 2 N, its weights rc_policy_load_heads' images.
#include "racecar_env.h"
#include "racecar_policy_math.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

#include <cmath>

namespace {

constexpr int FS = 233;                        // row stride of the feature tile (odd: the 32 rows on 32 banks)
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER, UNITS = RC_POLICY_UNITS, LD = RC_POLICY_LD400;
constexpr size_t kFitLds = (size_t)(2 * PM * XS + PM * FS + PM) * sizeof(float);
static_assert(kFitLds <= 160 * 1024, "X, Y, the feature tile and the output deltas");
// the gradient, the moments: the head's eight arrays one behind the other, [K_l + 1][400] = kernel | bias per hidden layer, [401][1]
constexpr int G1 = (FEAT + 1) * UNITS, G2 = G1 + (UNITS + 1) * UNITS, GO = G2 + (UNITS + 1) * UNITS, NG = GO + UNITS + 1;
static_assert(NG == 413601, "230 x 400 + 400 + 2 (400 x 400 + 400) + 400 + 1");
// a head of `depth` hidden layers: where its output layer's [401][1] lies in the gradient, and the gradient's length
__host__ __device__ constexpr int fit_go(int depth) { return depth == 3 ? GO : G2; }
__host__ __device__ constexpr int fit_ng(int depth) { return fit_go(depth) + UNITS + 1; }
static_assert(fit_ng(3) == NG && fit_ng(2) == 253201, "the value and pcont heads; the reward head");
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
    float *w[3], *b[3], *wout, *bout;          // the forward images (RcCriticDev's memory; the reward head: RcImagineDev's, two hidden
                                               // layers): [230 | 400][416], [416]; [400][32], [32]
    float *t1, *t2;                            // W1^T, W2^T [400][416], padding zero (the reward head: W1^T alone)
};

struct FitRowsCall {
    FitHeadDev h;
    const float *feat, *target, *weight;       // [N][230], [N], [N] or null
    int64_t n;
    float inv_n;
    int32_t pcont;
    float *act;                                // [6][N][416]: a1, a2, a3, delta1, delta2, delta3 (two hidden layers: [4][N][416])
    float *dout, *lterm;                       // [N] the output delta and the loss term
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

template <int TN>
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
            if (valid) L.g[(size_t)q * LD + j] = v;
        }
    }
}

__device__ __forceinline__ void fit_layer(const FitLayer &L, int wave, int lane, int64_t row0, int64_t n) {
    constexpr int n_tiles = LD / 32;
    const int mine = (n_tiles - wave + 3) / 4;          // tiles wave, wave + 4, ...: 4, 3, 3, 3
    if (mine == 4) fit_dense<4>(L, 32 * wave, lane, row0, n);
    else fit_dense<3>(L, 32 * wave, lane, row0, n);
}

// The rows kernel's body for a head of DEPTH hidden layers, 3 or 2.  Two layers are three without the third layer's forward product
// and without the transposed product that takes delta3 to delta2: the last hidden activation is then in Y, not in X.
template <int DEPTH>
__device__ __forceinline__ void fit_rows(const FitRowsCall &c) {
    static_assert(DEPTH == 2 || DEPTH == 3, "the reward head; the value and pcont heads");
    extern __shared__ float fit_lds[];
    float *X = fit_lds, *Y = fit_lds + PM * XS, *Z = fit_lds + 2 * PM * XS, *dl = Z + PM * FS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * PM, n = c.n;
    const size_t plane = (size_t)n * LD;
    float *a1 = c.act, *a2 = c.act + plane, *d1 = c.act + DEPTH * plane, *d2 = c.act + (DEPTH + 1) * plane;
    float *top = DEPTH == 3 ? X : Y, *dtop = c.act + (2 * DEPTH - 1) * plane;          // a_DEPTH's tile, delta_DEPTH's scratch

    for (int idx = tid; idx < PM * FS; idx += PT) {
        const int row = idx / FS, j = idx - row * FS;
        const int64_t q = row0 + row;
        Z[idx] = q < n && j < FEAT ? c.feat[(size_t)q * FEAT + j] : 0.0f;
    }
    __syncthreads();
    fit_layer(FitLayer{Z, FEAT, FS, c.h.w[0], c.h.b[0], X, nullptr, a1, FK_FORWARD}, wave, lane, row0, n);
    __syncthreads();
    fit_layer(FitLayer{X, UNITS, XS, c.h.w[1], c.h.b[1], Y, nullptr, a2, FK_FORWARD}, wave, lane, row0, n);
    __syncthreads();
    if constexpr (DEPTH == 3) {
        fit_layer(FitLayer{Y, UNITS, XS, c.h.w[2], c.h.b[2], X, nullptr, c.act + 2 * plane, FK_FORWARD}, wave, lane, row0, n);
        __syncthreads();
    }
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
        fit_layer(FitLayer{X, UNITS, XS, c.h.t2, nullptr, Y, nullptr, d2, FK_BACK_LDS}, wave, lane, row0, n);
        __syncthreads();
    }
    fit_layer(FitLayer{Y, UNITS, XS, c.h.t1, nullptr, nullptr, a1, d1, FK_BACK_GLOBAL}, wave, lane, row0, n);
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_fit_rows_kernel(FitRowsCall c) { fit_rows<3>(c); }
__global__ __launch_bounds__(PT) void rc_policy_fit_reward_rows_kernel(FitRowsCall c) { fit_rows<2>(c); }

struct FitWgradCall {
    const float *a[4];                         // a_{l-1} [N][lda]: the features, a1, a2, a3
    const float *d[4];                         // delta_l [N][ldd]: delta1, delta2, delta3, the output delta
    int32_t lda[4], ldd[4], k[4], nc[4];       // K_l = 230, 400, 400, 400; the columns 400, 400, 400, 1
    int32_t tile0[4], nt[4], goff[4];          // the layer's first workgroup, its column tiles, its place in the gradient
                                               // (two hidden layers: three entries; the fourth's tile0 is the grid, no workgroup is its)
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
    const int l = b >= c.tile0[3] ? 3 : (b >= c.tile0[2] ? 2 : (b >= c.tile0[1] ? 1 : 0));
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
    const int go = fit_go(depth);
    if (e >= go + UNITS + 1 || ctl->skipped) return;
    float *w, *wt = nullptr;
    if (e < go) {
        const int l = e < G1 ? 0 : (e < G2 ? 1 : 2);
        const int i = e - (l == 0 ? 0 : (l == 1 ? G1 : G2)), K = l == 0 ? FEAT : UNITS;
        const int k = i / UNITS, j = i - k * UNITS;
        w = k < K ? h.w[l] + (size_t)k * LD + j : h.b[l] + j;
        if (l > 0 && k < K) wt = (l == 1 ? h.t1 : h.t2) + (size_t)j * LD + k;
    } else {
        const int k = e - go;
        w = k < UNITS ? h.wout + (size_t)k * RC_POLICY_LDSMALL : h.bout;
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

// W [400][416] -> W^T [400][416], the padding columns zero
__global__ __launch_bounds__(PT) void rc_policy_fit_transpose_kernel(const float *w, float *t) {
    const int idx = blockIdx.x * PT + threadIdx.x;
    if (idx >= UNITS * LD) return;
    const int j = idx / LD, k = idx - j * LD;
    t[idx] = k < UNITS ? w[(size_t)k * LD + j] : 0.0f;
}

// ---- the optimizers of a handle and the entry points (include/racecar_hip.h, rc_policy_fit_*)
constexpr int kFitHeads = 3;                   // RC_POLICY_FIT_VALUE, _PCONT, _REWARD

struct RcFit {
    struct Head {
        float *mem = nullptr;                  // m [ng] | v [ng] | g [ng] | W1^T | W2^T (the reward head: W1^T alone)
        FitCtl *ctl = nullptr;
    } head[kFitHeads];
    float *scratch = nullptr;                  // [2 depth][rows][416] | the output delta [rows] | the loss terms [rows]: the heads share it
    size_t scratch_floats = 0;
};

namespace {

constexpr size_t kImage = (size_t)UNITS * LD;

constexpr int fit_depth(int head) { return head == RC_POLICY_FIT_REWARD ? 2 : 3; }
constexpr size_t fit_moment(int depth) { return ((size_t)fit_ng(depth) + 63) / 64 * 64; }

FitHeadDev fit_head(rc_env *env, int head) {
    const RcCriticDev &c = env->pol_c;
    const RcImagineDev &r = env->pol_i;
    FitHeadDev h{};
    if (head == RC_POLICY_FIT_REWARD) {
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
        h.t1 = env->fit->head[head].mem + 3 * fit_moment(fit_depth(head));
        if (fit_depth(head) == 3) h.t2 = h.t1 + kImage;
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
    if (!env->fit->head[0].mem && !env->fit->head[1].mem && !env->fit->head[2].mem) {
        if (env->fit->scratch) (void)hipFree(env->fit->scratch);
        delete env->fit;
        env->fit = nullptr;
    }
    return RC_OK;
}

const char *fit_head_name(int head) { return head == RC_POLICY_FIT_REWARD ? "reward" : (head == RC_POLICY_FIT_PCONT ? "pcont" : "value"); }
bool fit_head_known(int head) { return head == RC_POLICY_FIT_VALUE || head == RC_POLICY_FIT_PCONT || head == RC_POLICY_FIT_REWARD; }

}  // namespace

// rc_policy_load_critic, rc_policy_load, rc_policy_unload and rc_destroy close the critic's optimizers
int fit_release(rc_env *env) {
    const int rc = fit_close(env, RC_POLICY_FIT_VALUE);
    return rc ? rc : fit_close(env, RC_POLICY_FIT_PCONT);
}

// rc_policy_load_heads, rc_policy_load, rc_policy_unload and rc_destroy close the reward head's
int fit_release_reward(rc_env *env) { return fit_close(env, RC_POLICY_FIT_REWARD); }

extern "C" {

int rc_policy_fit_begin(rc_env *env, const rc_policy_fit_config *cfg) {
    if (!env || !cfg) return fail(RC_ERR_INVALID, "NULL argument");
    if (cfg->struct_size != sizeof(rc_policy_fit_config))
        return fail(RC_ERR_INVALID, "rc_policy_fit_config.struct_size %u != %zu", cfg->struct_size, sizeof(rc_policy_fit_config));
    if (!fit_head_known(cfg->head)) return fail(RC_ERR_INVALID, "rc_policy_fit_begin: unknown head %d", cfg->head);
    const int head = cfg->head, depth = fit_depth(head);
    if (!fit_head(env, head).wout)
        return fail(RC_ERR_INVALID, "rc_policy_fit_begin: no %s head is loaded (%s)", fit_head_name(head),
                    head == RC_POLICY_FIT_REWARD ? "rc_policy_load_heads" : "rc_policy_load_critic");
    int rc = fit_close(env, head);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipFuncSetAttribute((const void *)rc_policy_fit_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitLds));
    HIP_TRY(hipFuncSetAttribute((const void *)rc_policy_fit_reward_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitLds));
    if (!env->fit) env->fit = new RcFit();
    RcFit::Head &o = env->fit->head[head];
    const size_t kMoment = fit_moment(depth), floats = 3 * kMoment + (size_t)(depth - 1) * kImage;
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
    hipLaunchKernelGGL(rc_policy_fit_transpose_kernel, dim3(blocks), dim3(PT), 0, env->stream, (const float *)h.w[1], h.t1);
    if (depth == 3) hipLaunchKernelGGL(rc_policy_fit_transpose_kernel, dim3(blocks), dim3(PT), 0, env->stream, (const float *)h.w[2], h.t2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(env->stream));             // (`init` goes out of scope)
    return RC_OK;
}

int rc_policy_fit_step(rc_env *env, const rc_policy_fit_args *a) {
    if (!env || !a) return fail(RC_ERR_INVALID, "NULL argument");
    if (a->struct_size != sizeof(rc_policy_fit_args))
        return fail(RC_ERR_INVALID, "rc_policy_fit_args.struct_size %u != %zu", a->struct_size, sizeof(rc_policy_fit_args));
    if (!fit_head_known(a->head)) return fail(RC_ERR_INVALID, "rc_policy_fit_step: unknown head %d", a->head);
    const int head = a->head, depth = fit_depth(head), ng = fit_ng(depth);
    if (!env->fit || !env->fit->head[head].mem)
        return fail(RC_ERR_INVALID, "rc_policy_fit_step: no optimizer is open for the %s head (rc_policy_fit_begin)", fit_head_name(head));
    if (!a->features || !a->target) return fail(RC_ERR_INVALID, "rc_policy_fit_step: %s is NULL", !a->features ? "features" : "target");
    if (a->rows < 1 || a->rows > (int64_t)INT32_MAX) return fail(RC_ERR_INVALID, "rc_policy_fit_step: rows %lld is outside [1, 2^31)", (long long)a->rows);
    const float hyper[5] = {a->lr, a->clip, a->beta1, a->beta2, a->epsilon};
    const char *names[5] = {"lr", "clip", "beta1", "beta2", "epsilon"};
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(hyper[i]) || hyper[i] < 0.0f)
            return fail(RC_ERR_INVALID, "rc_policy_fit_step: %s %g is not a finite number >= 0", names[i], (double)hyper[i]);
    if (a->beta1 >= 1.0f || a->beta2 >= 1.0f)
        return fail(RC_ERR_INVALID, "rc_policy_fit_step: beta1 %g, beta2 %g: both must lie in [0, 1)", (double)a->beta1, (double)a->beta2);
    HIP_TRY(hipSetDevice(env->cfg.device));
    RcFit &f = *env->fit;
    const int64_t n = a->rows;
    const size_t need = (size_t)n * (2 * depth * LD + 2);
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
    FitRowsCall r{};
    r.h = fit_head(env, head);
    r.feat = a->features; r.target = a->target; r.weight = a->weight;
    r.n = n;
    r.inv_n = 1.0f / (float)n;
    r.pcont = head == RC_POLICY_FIT_PCONT;
    r.act = f.scratch;
    r.dout = f.scratch + 2 * depth * plane;
    r.lterm = r.dout + n;
    FitWgradCall w{};
    const int goff[4] = {0, G1, G2, GO};
    int tiles = 0;
    for (int l = 0; l <= depth; ++l) {          // layer l's input a_l (the features, a1 ..) and delta_{l+1} (.., the output delta)
        const bool out = l == depth;
        w.a[l] = l == 0 ? a->features : r.act + (size_t)(l - 1) * plane;
        w.d[l] = out ? r.dout : r.act + (size_t)(depth + l) * plane;
        w.lda[l] = l == 0 ? FEAT : LD;
        w.ldd[l] = out ? 1 : LD;
        w.k[l] = l == 0 ? FEAT : UNITS;
        w.nc[l] = out ? 1 : UNITS;
        w.tile0[l] = tiles;
        w.nt[l] = (w.nc[l] + 31) / 32;
        w.goff[l] = goff[l];
        tiles += (w.k[l] + 1 + 31) / 32 * w.nt[l];
    }
    for (int l = depth + 1; l < 4; ++l) w.tile0[l] = tiles;
    w.g = g;
    w.n = n;
    KernelTimer t;
    int rc = t.begin(env, RC_K_POLICY, true);
    if (rc) return rc;
    const dim3 row_blocks((unsigned)((n + PM - 1) / PM));
    if (depth == 3) hipLaunchKernelGGL(rc_policy_fit_rows_kernel, row_blocks, dim3(PT), (uint32_t)kFitLds, env->stream, r);
    else hipLaunchKernelGGL(rc_policy_fit_reward_rows_kernel, row_blocks, dim3(PT), (uint32_t)kFitLds, env->stream, r);
    hipLaunchKernelGGL(rc_policy_fit_wgrad_kernel, dim3((unsigned)tiles), dim3(PT), 0, env->stream, w);
    hipLaunchKernelGGL(rc_policy_fit_sums_kernel, dim3(SUM_BLOCKS), dim3(PT), 0, env->stream, (const float *)g, ng, (const float *)r.lterm, n, o.ctl);
    hipLaunchKernelGGL(rc_policy_fit_scale_kernel, dim3(1), dim3(64), 0, env->stream, o.ctl, n, a->lr, a->clip, a->beta1, a->beta2, a->status);
    hipLaunchKernelGGL(rc_policy_fit_apply_kernel, dim3((ng + PT - 1) / PT), dim3(PT), 0, env->stream, r.h, depth, (const float *)g, m, v,
                       (const FitCtl *)o.ctl, a->beta1, a->beta2, 1.0f - a->beta1, 1.0f - a->beta2, a->epsilon);
    // rc_policy_dream_grad keeps transposed copies of the reward head's two hidden layers: its next call makes them again, on the stream
    if (head == RC_POLICY_FIT_REWARD) env->dgrad_reward_stale = true;
    HIP_TRY(hipGetLastError());
    return t.end();
}

int rc_policy_fit_end(rc_env *env, int32_t head) {
    if (!env) return fail(RC_ERR_INVALID, "env is NULL");
    if (!fit_head_known(head)) return fail(RC_ERR_INVALID, "rc_policy_fit_end: unknown head %d", head);
    return fit_close(env, head);
}

}  // extern "C"
