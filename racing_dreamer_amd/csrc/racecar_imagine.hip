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
#include "racecar_rollout.h"

namespace {

constexpr size_t kLdsBytes = RO_LDS_XYZ + PM * sizeof(int);
constexpr size_t kLdsBytesSampled = kLdsBytes + RO_LDS_DRAWS;

enum { IK_STOCH = RO_OUT, IK_ACTION, IK_REWARD };

template <bool SAMPLED>
__device__ __forceinline__ void im_imagine(const RcImagineCall &c) {
    extern __shared__ float im_lds[];
    const RoLds lds = ro_carve(im_lds);
    float *X = lds.X, *Y = lds.Y, *Z = lds.Z;
    int *cars = (int *)lds.rest;
    float *normals = (float *)(cars + PM);                   // [32][PN]   (sampled only)
    uint32_t *key = (uint32_t *)(normals + PM * PN);         // [32][4]    global env, episode, agent step, slot
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
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
        // the row's place in the caller's [n_cars][H] arrays at this step
        auto at_step = [&](int row) { return cars[row] >= 0 ? (int64_t)cars[row] * c.horizon + t : (int64_t)-1; };
        if (t >= 0) {
            if constexpr (SAMPLED) {
                ro_stage_normals(normals, [&](int row) { return cars[row] >= 0; }, [&](int row, uint32_t blk, float (&n)[4]) {
                    const uint32_t *k = key + 4 * row;
                    pm_imagine_normal_block(k[0], k[1], k[2], k[3], (uint32_t)t, blk, c.rows.seed_lo, c.rows.seed_hi, n);
                }, !open_loop, tid);
            }
            if (open_loop) ro_stage_actions(c.actions_in, c.actions, at_step, Z, tid);
            __syncthreads();
        }
        // mode `mean`: tanh of the actor's mean; the head's one column: t < 0 is the starting feature
        auto out = [&](const RoLayer &L, int row, int j, float v) {
            const int car = cars[row];
            if (L.kind == IK_ACTION) {
                const float *hn = c.w.hnorm;
                const float act = hn ? pm_action_normalized(v, hn[j], hn[2 + j], hn[4 + j], hn[6 + j]) : pm_action_plain(v);
                L.d[row * ZS + j] = act;
                if (car >= 0 && c.actions) c.actions[((size_t)car * c.horizon + t) * 2 + j] = act;
            } else if (car >= 0) {
                L.g[t < 0 ? (size_t)car : (size_t)car * c.horizon + t] = v;
            }
        };
        const int first = t < 0 ? 8 : (open_loop ? 5 : 0), last = (t < 0 || head) ? 11 : 8;
#pragma unroll 1
        for (int layer = first; layer < last; ++layer) {
            RoLayer L;
            switch (layer) {
            case 0: L = ro_first(Z, c.w.h_w[0], c.w.h_b[0], X); break;
            case 1: L = ro_hidden(X, c.w.h_w[1], c.w.h_b[1], Y); break;
            case 2: L = ro_hidden(Y, c.w.h_w[2], c.w.h_b[2], X); break;
            case 3: L = ro_hidden(X, c.w.h_w[3], c.w.h_b[3], Y); break;
            case 4: L = ro_actor_out<SAMPLED>(Y, c.w, c.ws, Z, IK_ACTION); break;
            case 5: L = ro_img1(Z, c.w, X); break;
            case 6: L = ro_img2(Y, c.wi, X); break;
            case 7: L = ro_img3(X, c.wi, Z, SAMPLED ? IK_STOCH : RO_STORE_Z); break;
            case 8: L = ro_first(Z, c.wi.rh_w[0], c.wi.rh_b[0], X); break;
            case 9: L = ro_hidden(X, c.wi.rh_w[1], c.wi.rh_b[1], Y); break;
            default: L = ro_column(Y, c.wi.rout_w, c.wi.rout_b, IK_REWARD, t < 0 ? c.reward_start : c.reward); break;
            }
            if (layer == 6) ro_commit_deter(Y, Z, tid);
            if (SAMPLED && (layer == 4 || layer == 7)) {
                if (wave == 0) ro_dense_pair(L, lane, [&](int row, int j, float mean, float raw) {
                    float v;
                    if (L.kind == IK_STOCH) {
                        v = ro_sampled_stoch(mean, raw, normals[row * PN + j]);
                    } else {
                        float mu, sd;
                        pm_actor_dist(mean, raw, c.ws.hnorm4, j, mu, sd);
                        v = pm_tanh(fmaf(sd, normals[row * PN + 32 + j], mu));
                        const int car = cars[row];
                        if (car >= 0 && c.actions) c.actions[((size_t)car * c.horizon + t) * 2 + j] = v;
                    }
                    L.d[row * ZS + j] = v;
                });
            } else ro_layer(L, wave, lane, out);
            __syncthreads();
            if (layer != 5) continue;
            ro_gru(c.w, X, Z, Y, wave, lane);
            __syncthreads();
        }
        if (t >= 0 && c.features) ro_store_features(c.features, at_step, Z, tid);
    }
}

}  // namespace

__global__ __launch_bounds__(PT) void rc_policy_imagine_kernel(RcImagineCall c) { im_imagine<false>(c); }
__global__ __launch_bounds__(PT) void rc_policy_imagine_sampled_kernel(RcImagineCall c) { im_imagine<true>(c); }

hipError_t rck_imagine_prepare() { return ro_prepare(rc_policy_imagine_kernel, rc_policy_imagine_sampled_kernel, kLdsBytes, kLdsBytesSampled); }

hipError_t rck_launch_imagine(const RcImagineCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    return ro_launch(c.sample ? rc_policy_imagine_sampled_kernel : rc_policy_imagine_kernel, c.rows.n_active,
                     c.sample ? kLdsBytesSampled : kLdsBytes, c, start, stop, s);
}
