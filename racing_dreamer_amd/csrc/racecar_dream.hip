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
#include "racecar_rollout.h"

namespace {

// behind X, Y, Z per row: the output row s K + k and the state row of its start (int64, -1 past the end), the return
constexpr size_t kLdsBytes = RO_LDS_XYZ + PM * (2 * sizeof(int64_t) + sizeof(float));
constexpr size_t kLdsBytesSampled = kLdsBytes + RO_LDS_DRAWS;

enum { DK_REWARD = RO_OUT };

template <bool SAMPLED>
__device__ __forceinline__ void dr_dream(const RcDreamCall &c) {
    extern __shared__ float dr_lds[];
    const RoLds lds = ro_carve(dr_lds);
    float *X = lds.X, *Y = lds.Y, *Z = lds.Z;
    int64_t *out_row = (int64_t *)lds.rest;                  // [32] s K + k of the row in the caller's arrays, -1 past the end
    int64_t *lat_row = out_row + PM;                         // [32]
    float *ret = (float *)(lat_row + PM);                    // [32] the return so far
    uint32_t *key = (uint32_t *)(ret + PM);                  // [32][4] start id lo, hi, candidate, -   (sampled only)
    float *normals = (float *)(key + 4 * PM);                // [32][PN]                                 (sampled only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
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
    ro_load_latent_rows(c.state, [&](int row) { return lat_row[row]; }, Z, tid);
    __syncthreads();

    const bool head = c.ret != nullptr || c.reward != nullptr;
    float weight = 1.0f;
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        if constexpr (SAMPLED) {
            ro_stage_normals(normals, [&](int row) { return out_row[row] >= 0; }, [&](int row, uint32_t blk, float (&n)[4]) {
                const uint32_t *k = key + 4 * row;
                pm_dream_normal_block(k[0], k[1], k[2], (uint32_t)t, blk, c.seed_lo, c.seed_hi, n);
            }, false, tid);
        }
        ro_stage_actions(c.actions_in, nullptr, [&](int row) { return out_row[row] >= 0 ? out_row[row] * H + t : (int64_t)-1; }, Z, tid);
        __syncthreads();
        // the head's one column: this lane alone owns its 16 rows' returns
        auto out = [&](const RoLayer &L, int row, int, float v) {
            const int64_t q = out_row[row];
            if (q < 0) return;
            if (L.g) L.g[(size_t)q * H + t] = v;
            ret[row] = fmaf(weight, v, ret[row]);
        };
        const int last = head ? 6 : 3;
#pragma unroll 1
        for (int layer = 0; layer < last; ++layer) {
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
            if (SAMPLED && layer == 2) {
                if (wave == 0) ro_dense_pair(L, lane, [&](int row, int j, float mean, float raw) {
                    L.d[row * ZS + j] = ro_sampled_stoch(mean, raw, normals[row * PN + j]);
                });
            } else ro_layer(L, wave, lane, out);
            __syncthreads();
            if (layer != 0) continue;
            ro_gru(c.w, X, Z, Y, wave, lane);
            __syncthreads();
        }
        weight = weight * c.discount;
    }
    // what leaves the CU at the end: the returns, and the feature [stoch', deter'] after step H - 1 (the last layer's barrier is behind us)
    if (c.ret && tid < PM && out_row[tid] >= 0) c.ret[out_row[tid]] = ret[tid];
    if (c.final_feature) ro_store_features(c.final_feature, [&](int row) { return out_row[row]; }, Z, tid);
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_dream_kernel(RcDreamCall c) { dr_dream<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_dream_sampled_kernel(RcDreamCall c) { dr_dream<true>(c); }

hipError_t rck_dream_prepare() { return ro_prepare(rc_policy_dream_kernel, rc_policy_dream_sampled_kernel, kLdsBytes, kLdsBytesSampled); }

hipError_t rck_launch_dream(const RcDreamCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    return ro_launch(c.sample ? rc_policy_dream_sampled_kernel : rc_policy_dream_kernel, c.n_rows, c.sample ? kLdsBytesSampled : kLdsBytes,
                     c, start, stop, s);
}
