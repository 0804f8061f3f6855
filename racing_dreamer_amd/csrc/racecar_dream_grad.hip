// rc_policy_dream_grad: the vector-Jacobian product of the open-loop dream - the derivative of
// rc_policy_dream_ahead's return with respect to the raw action sequence and to the start latent, through the reward head
// (dreamer/models.py:301-318 DenseDecoder) and the prior step (models.py:369-380 `RSSM.img_step`), in the binary32 arithmetic of
// tests/policy_dream_grad_spec.c; the device equals it bit for bit.  No weight gradient, no reduction across rows, no atomics: rows
// are independent.
//
// ONE kernel per mode, one launch per chunk of rows: the geometry is rc_policy_dream_kernel's (racecar_dream.hip: 32 (start,
// candidate) rows per workgroup, four waves, X and Y [32][417] and the latent Z [32][233] in LDS, the layers of racecar_rollout.h).
//   forward   item 19's step, unchanged in arithmetic, draws and keying; what the backward needs of step t goes to the row's
//             stash in global memory as the layer that made it is read by the next: per (row, t) RC_DREAM_GRAD_STASH floats =
//             x1 200 | z, r, c, hh 4 x 200 | h 200 | x2 200 | raw std 30 (+ 10) | a1 400 | a2 400.  A workgroup reads back only
//             what its own waves wrote, a barrier later.
//   backward  t = H - 1 .. 0 on the same tiles; Z holds the carry (deter 200 | stoch 30), every product is a k-ascending MFMA
//             chain from zero over a transposed weight image (RcDreamGradDev), the normals of `sample` mode are drawn again from
//             the step's key.  Nine barriers per step.
// The host cuts the rows into chunks against the handle's stash (dream_grad_run): a row's numbers depend on nothing but the row.
// The record's layout and the transposed-product helpers are racecar_dream_grad.h's, shared with racecar_returns_grad.hip.
#include "racecar_dream_grad.h"

namespace {

constexpr int SW = RC_DREAM_GRAD_STASH;
constexpr int MAX_H = RC_POLICY_IMAGINE_MAX_HORIZON;
// behind X, Y, Z: per row the output row s K + k and the state row of its start (int64, -1 past the end) and the return; the
// forward's weight sequence w_t; sampled: the draw's key and a step's normals
constexpr size_t kLdsBytes = RO_LDS_XYZ + PM * (2 * sizeof(int64_t) + sizeof(float)) + MAX_H * sizeof(float);
constexpr size_t kLdsBytesSampled = kLdsBytes + RO_LDS_DRAWS;
static_assert(kLdsBytesSampled <= 160 * 1024, "X, Y, Z, the rows' records, the weight sequence, the key and the normals");

enum { DK_REWARD = RO_OUT };

template <bool SAMPLED>
__device__ __forceinline__ void dg_dream_grad(const RcDreamGradCall &g) {
    extern __shared__ float dg_lds[];
    const RcDreamCall &c = g.d;
    const RoLds lds = ro_carve(dg_lds);
    float *X = lds.X, *Y = lds.Y, *Z = lds.Z;
    int64_t *out_row = (int64_t *)lds.rest;                  // [32] s K + k of the row in the caller's arrays, -1 past the end
    int64_t *lat_row = out_row + PM;                         // [32]
    float *ret = (float *)(lat_row + PM);                    // [32] the return so far
    float *wts = ret + PM;                                   // [64] w_t, the forward's own sequence
    uint32_t *key = (uint32_t *)(wts + MAX_H);               // [32][4] start id lo, hi, candidate, -   (sampled only)
    float *normals = (float *)(key + 4 * PM);                // [32][PN]                                 (sampled only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = g.row_begin + (int64_t)blockIdx.x * PM;
    const int H = c.horizon;
    const size_t stride = (size_t)H * SW;                    // a row's stash
    float *stash = g.stash + (size_t)blockIdx.x * PM * stride;

    if (tid < PM) {
        const int64_t q = row0 + tid;
        int64_t o = -1, l = -1;
        uint64_t id = 0;
        uint32_t k = 0;
        if (q < c.n_rows) {
            const int64_t s = q / c.candidates;
            k = (uint32_t)(q - s * c.candidates);
            if (c.live) {
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
    ro_load_latent_rows(c.state, [&](int row) { return lat_row[row]; }, Z, tid);
    __syncthreads();

    auto stage_normals = [&](int t) {
        ro_stage_normals(normals, [&](int row) { return out_row[row] >= 0; }, [&](int row, uint32_t blk, float (&n)[4]) {
            const uint32_t *k = key + 4 * row;
            pm_dream_normal_block(k[0], k[1], k[2], (uint32_t)t, blk, c.seed_lo, c.seed_hi, n);
        }, false, tid);
    };

    // ---- forward: racecar_dream.hip's loop, the head always run
    float weight = 1.0f;
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        float *st = stash + (size_t)t * SW;
        if constexpr (SAMPLED) stage_normals(t);
        ro_stage_actions(c.actions_in, nullptr, [&](int row) { return out_row[row] >= 0 ? out_row[row] * H + t : (int64_t)-1; }, Z, tid);
        if (tid == 0) wts[t] = weight;
        __syncthreads();
        auto out = [&](const RoLayer &L, int row, int, float v) {
            const int64_t q = out_row[row];
            if (q < 0) return;
            if (L.g) L.g[(size_t)q * H + t] = v;
            ret[row] = fmaf(weight, v, ret[row]);
        };
#pragma unroll 1
        for (int layer = 0; layer < 6; ++layer) {
            RoLayer L;
            switch (layer) {
            case 0: L = ro_img1(Z, c.w, X); break;
            case 1: L = ro_img2(Y, c.wi, X); break;
            case 2: L = ro_img3(X, c.wi, Z); break;
            case 3: L = ro_first(Z, c.wi.rh_w[0], c.wi.rh_b[0], X); break;
            case 4: L = ro_hidden(X, c.wi.rh_w[1], c.wi.rh_b[1], Y); break;
            default: L = ro_column(Y, c.wi.rout_w, c.wi.rout_b, DK_REWARD, c.reward); break;
            }
            if (layer == 1) ro_commit_deter(Y, Z, tid);
            // the input of this layer is what the layer before left: kept while it is read
            if (layer == 2) dg_keep(X, XS, RC_POLICY_DETER, st + S_X2, stride, tid);
            if (layer == 4) dg_keep(X, XS, RC_POLICY_UNITS, st + S_A1, stride, tid);
            if (layer == 5) dg_keep(Y, XS, RC_POLICY_UNITS, st + S_A2, stride, tid);
            if (SAMPLED && layer == 2) {
                if (wave == 0) ro_dense_pair(L, lane, [&](int row, int j, float mean, float raw) {
                    L.d[row * ZS + j] = ro_sampled_stoch(mean, raw, normals[row * PN + j]);
                    st[row * stride + S_RAW + j] = raw;
                });
            } else ro_layer(L, wave, lane, out);
            __syncthreads();
            if (layer != 0) continue;
            dg_keep(X, XS, RC_POLICY_DETER, st + S_X1, stride, tid);
            dg_keep(Z, ZS, RC_POLICY_DETER, st + S_H, stride, tid);
            dg_gru(c.w, X, Z, Y, st, stride, wave, lane);
            __syncthreads();
        }
        weight = weight * c.discount;
    }
    if (c.ret && tid < PM && out_row[tid] >= 0) c.ret[out_row[tid]] = ret[tid];
    if (!g.grad_actions && !g.grad_state) return;

    // ---- backward: Z = the carry, deter at [0, 200), stoch at [200, 230)
    for (int idx = tid; idx < PM * ZS; idx += PT) Z[idx] = 0.0f;
    __syncthreads();
    const int cc = lane & 31, half = lane >> 5;
#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        const float *st = stash + (size_t)t * SW;
        // 1. head: delta a2 -> X.  (Here and in the GRU's deltas below a thread asks for the stash entries of U elements before it
        // uses the first: one wave per SIMD hides no latency by itself.)
        {
            constexpr int U = 10;
            static_assert(PM * RC_POLICY_UNITS % (PT * U) == 0, "whole batches");
            const float wt = wts[t];
#pragma unroll 1
            for (int base = tid; base < PM * RC_POLICY_UNITS; base += PT * U) {
                float a2[U], wo[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = base + u * PT, row = idx / RC_POLICY_UNITS, j = idx - row * RC_POLICY_UNITS;
                    a2[u] = st[row * stride + S_A2 + j];
                    wo[u] = c.wi.rout_w[(size_t)j * RC_POLICY_LDSMALL];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = base + u * PT, row = idx / RC_POLICY_UNITS, j = idx - row * RC_POLICY_UNITS;
                    X[row * XS + j] = fmaf(wt, wo[u], 0.0f) * dg_elu_grad(a2[u]);
                }
            }
        }
        if constexpr (SAMPLED) stage_normals(t);
        __syncthreads();
        // delta a1 = (delta a2 rh1^T) elu'(a1) -> Y
        dg_layer400(X, RC_POLICY_UNITS, g.wt.rh1_t, wave, lane,
                    [&](int row, int j, float v) { Y[row * XS + j] = v * dg_elu_grad(st[row * stride + S_A1 + j]); });
        __syncthreads();
        // 2. g = g_head + carry, in place (feature column j: stoch | deter)
        dg_layer256(Y, RC_POLICY_UNITS, nullptr, 0, g.wt.rh0_t, FEAT, wave, lane, [&](int row, int j, float v) {
            float *z = Z + row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH);
            *z = v + *z;
        });
        __syncthreads();
        // 3. stoch': [delta mean | delta raw] -> X[0, 60)
        for (int idx = tid; idx < PM * RC_POLICY_STOCH; idx += PT) {
            const int row = idx / RC_POLICY_STOCH, j = idx - row * RC_POLICY_STOCH;
            const float gs = Z[row * ZS + Z_STOCH + j];
            X[row * XS + j] = gs;
            if constexpr (SAMPLED) X[row * XS + RC_POLICY_STOCH + j] = (gs * normals[row * PN + j]) * pm_sigmoid(st[row * stride + S_RAW + j]);
        }
        __syncthreads();
        // 4. img3: delta x2 -> Y[0, 200)
        dg_layer256(X, SAMPLED ? 2 * RC_POLICY_STOCH : RC_POLICY_STOCH, nullptr, 0, g.wt.img3_t, RC_POLICY_DETER, wave, lane,
                    [&](int row, int j, float v) { Y[row * XS + j] = v * dg_elu_grad(st[row * stride + S_X2 + j]); });
        __syncthreads();
        // 5. img2: delta d = (delta x2 img2^T) + g_deter, in place
        dg_layer256(Y, RC_POLICY_DETER, nullptr, 0, g.wt.img2_t, RC_POLICY_DETER, wave, lane, [&](int row, int j, float v) {
            float *z = Z + row * ZS + j;
            *z = v + *z;
        });
        __syncthreads();
        // 6. GRU: Y = [delta z | delta r], X = [delta c | delta hh]
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
            pm_gemm<2>(acc, Y + cc * XS + half, RC_POLICY_DETER, g.wt.gruk_t + (size_t)half * LDT + cc, LDT, col);
            pm_gemm<2>(acc, X + cc * XS + half, RC_POLICY_DETER / 2, g.wt.gruk_t + (size_t)(2 * RC_POLICY_DETER + half) * LDT + cc, LDT, col);
            // carry_deter = fmaf(delta d, z, [dz | dr | dhh] gru_r^T), in place
            dg_layer256(Y, 2 * RC_POLICY_DETER, X + RC_POLICY_DETER, RC_POLICY_DETER, g.wt.grur_t, RC_POLICY_DETER, wave, lane, [&](int row, int j, float v) {
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
        // 7. img1: delta in -> the carry's stoch, and the actions' gradient where the raw action lies in [-1, 1]
        if (wave == 0)
            dg_dense<1>(X, RC_POLICY_DETER, nullptr, 0, XS, g.wt.img1_t, 32, 32, 0, lane, [&](int row, int j, float v) {
                if (j < RC_POLICY_STOCH) {
                    Z[row * ZS + Z_STOCH + j] = v;
                    return;
                }
                const int64_t q = out_row[row];
                if (q < 0 || !g.grad_actions) return;
                const size_t at = ((size_t)q * H + t) * 2 + (j - RC_POLICY_STOCH);
                const float a = c.actions_in[at];
                g.grad_actions[at] = (a >= -1.0f && a <= 1.0f) ? v : 0.0f;
            });
        __syncthreads();
    }
    if (g.grad_state) ro_store_features(g.grad_state, [&](int row) { return out_row[row]; }, Z, tid);
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_dream_grad_kernel(RcDreamGradCall g) { dg_dream_grad<false>(g); }
__global__ __launch_bounds__(PT) void rc_policy_dream_grad_sampled_kernel(RcDreamGradCall g) { dg_dream_grad<true>(g); }

// W [..][src_ld] -> W^T [k_n][dst_ld]: row k of the image is column (k / group) group_ld + k % group of W, its first n entries W's
// rows, the padding zero
__global__ __launch_bounds__(PT) void rc_policy_dream_grad_transpose_kernel(const float *w, int src_ld, int group, int group_ld, int k_n, int n,
                                                                            int dst_ld, float *t) {
    const int idx = blockIdx.x * PT + threadIdx.x;
    if (idx >= k_n * dst_ld) return;
    const int k = idx / dst_ld, i = idx - k * dst_ld;
    const int g = k / group;
    t[idx] = i < n ? w[(size_t)i * src_ld + g * group_ld + (k - g * group)] : 0.0f;
}

void rck_dream_grad_transpose(const float *w, int src_ld, int group, int group_ld, int k_n, int n, int dst_ld, float *t, hipStream_t s) {
    const unsigned blocks = (unsigned)(((size_t)k_n * dst_ld + PT - 1) / PT);
    hipLaunchKernelGGL(rc_policy_dream_grad_transpose_kernel, dim3(blocks), dim3(PT), 0, s, w, src_ld, group, group_ld, k_n, n, dst_ld, t);
}

hipError_t rck_dream_grad_prepare() {
    return ro_prepare(rc_policy_dream_grad_kernel, rc_policy_dream_grad_sampled_kernel, kLdsBytes, kLdsBytesSampled);
}

// ---- the handle's images and stash, and the chunks of a call
struct RcDreamGrad {
    float *images = nullptr;                   // the seven transposed images, one allocation
    RcDreamGradDev wt{};
    float *stash = nullptr;
    size_t stash_floats = 0;
};

namespace {

constexpr size_t kStashBudget = (size_t)1 << 30;          // bytes: the stash never grows beyond it

struct TImage { const float *RcDreamGradDev::*dst; int k_n, n, dst_ld, src_ld, group, group_ld; };

}  // namespace

int dream_grad_release(rc_env *env) {
    if (!env->dgrad) return RC_OK;
    HIP_TRY(hipSetDevice(env->cfg.device));
    HIP_TRY(hipStreamSynchronize(env->stream));
    if (env->dgrad->images) (void)hipFree(env->dgrad->images);
    if (env->dgrad->stash) (void)hipFree(env->dgrad->stash);
    delete env->dgrad;
    env->dgrad = nullptr;
    return RC_OK;
}

int dream_grad_run(rc_env *env, RcDreamGradCall &c, int64_t chunk_rows) {
    const int D = RC_POLICY_DETER, U = RC_POLICY_UNITS, NS = RC_POLICY_STOCH;
    const TImage table[7] = {
        {&RcDreamGradDev::img1_t, D, 32, 32, RC_POLICY_LD200, D, 0},
        {&RcDreamGradDev::gruk_t, 3 * D, D, LDT, RC_POLICY_LDGRU, D, RC_POLICY_LD200},
        {&RcDreamGradDev::grur_t, 3 * D, D, LDT, RC_POLICY_LDGRU, D, RC_POLICY_LD200},
        {&RcDreamGradDev::img2_t, D, D, LDT, RC_POLICY_LD200, D, 0},
        {&RcDreamGradDev::img3_t, 2 * NS, D, LDT, RC_POLICY_LDPAIR, NS, 32},
        {&RcDreamGradDev::rh0_t, U, FEAT, LDT, RC_POLICY_LD400, U, 0},
        {&RcDreamGradDev::rh1_t, U, U, RC_POLICY_LD400, RC_POLICY_LD400, U, 0},
    };
    const float *src[7] = {env->pol.img1_w, env->pol.gru_k, env->pol.gru_r, env->pol_i.img2_w, env->pol_i.img3_w, env->pol_i.rh_w[0], env->pol_i.rh_w[1]};
    auto transpose = [&](int i, float *dst) {
        const TImage &im = table[i];
        rck_dream_grad_transpose(src[i], im.src_ld, im.group, im.group_ld, im.k_n, im.n, im.dst_ld, dst, env->stream);
    };
    if (!env->dgrad) {
        // the first call after the weights were loaded: the transposed images, built on the device
        size_t at[7], total = 0;
        for (int i = 0; i < 7; ++i) {
            at[i] = total;
            total += ((size_t)table[i].k_n * table[i].dst_ld + 63) / 64 * 64;
        }
        RcDreamGrad *d = new RcDreamGrad();
        const hipError_t e = hipMalloc((void **)&d->images, total * sizeof(float));
        if (e != hipSuccess) {
            delete d;
            return fail(RC_ERR_HIP, "rc_policy_dream_grad: %s", hipGetErrorString(e));
        }
        env->dgrad = d;
        for (int i = 0; i < 7; ++i) {
            float *dst = d->images + at[i];
            transpose(i, dst);
            d->wt.*(table[i].dst) = dst;
        }
        HIP_TRY(hipGetLastError());
    } else if (env->dgrad_reward_stale) {
        // rc_policy_fit_step moved the reward head since: its two images again, in place and in stream order behind that step
        for (int i = 5; i < 7; ++i) transpose(i, const_cast<float *>(env->dgrad->wt.*(table[i].dst)));
        HIP_TRY(hipGetLastError());
    }
    env->dgrad_reward_stale = false;
    RcDreamGrad &d = *env->dgrad;
    const int64_t n_rows = c.d.n_rows, H = c.d.horizon;
    const size_t row_floats = (size_t)H * SW;
    const int64_t padded = (n_rows + PM - 1) / PM * PM;        // n_rows < 2^31
    int64_t chunk = (int64_t)(kStashBudget / (row_floats * sizeof(float))) / PM * PM;          // H = 15: 7 968 rows; H = 64: 1 856
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
        if (e != hipSuccess) return fail(RC_ERR_HIP, "rc_policy_dream_grad: the stash of %zu bytes: %s", need * sizeof(float), hipGetErrorString(e));
        d.stash_floats = need;
    }
    c.wt = d.wt;
    c.stash = d.stash;
    KernelTimer t;
    const int rc = t.begin(env, RC_K_POLICY, true);
    if (rc) return rc;
    for (int64_t begin = 0; begin < n_rows; begin += chunk) {
        RcDreamGradCall k = c;
        k.row_begin = begin;
        k.d.n_rows = begin + chunk < n_rows ? begin + chunk : n_rows;
        const unsigned blocks = (unsigned)((k.d.n_rows - begin + PM - 1) / PM);
        if (c.d.sample) hipLaunchKernelGGL(rc_policy_dream_grad_sampled_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytesSampled, env->stream, k);
        else hipLaunchKernelGGL(rc_policy_dream_grad_kernel, dim3(blocks), dim3(PT), (uint32_t)kLdsBytes, env->stream, k);
    }
    const hipError_t e = hipGetLastError();
    const int rc_end = t.end();                             // (also after a refused launch: the event pair goes back to the handle)
    if (e != hipSuccess) return fail(RC_ERR_HIP, "rc_policy_dream_grad: %s", hipGetErrorString(e));
    return rc_end;
}
