// The latent-step engine of the rollout units (racecar_imagine.hip, racecar_dream.hip, racecar_dream_grad.hip, racecar_returns.hip,
// racecar_observe.hip): what a workgroup of racecar_policy_tiles.h needs to carry 32 latents through RSSM.img_step and the heads
// that read them.  The latent lives in Z [32][233] = deter 200 | stoch 30 | action 2 behind the activation buffers X and Y.  A
// unit keeps its call record, its row mapping and draw key, its schedule (which layers run at step t) and its output epilogues;
// the layer record, the dense wrapper and its ladder, the GRU, the row staging and the host tail are here, once.  The agent
// (racecar_policy.hip) is not a client: its GRU reads h from Y and it is the one kernel on the closed-loop path.
// Not part of the public interface.
#pragma once
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

namespace {

constexpr int ZS = 233;                        // row stride of Z (41 mod 64, odd: the 32 rows on 32 banks)
constexpr int Z_STOCH = RC_POLICY_DETER, Z_ACTION = RC_POLICY_DETER + RC_POLICY_STOCH;
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
constexpr size_t RO_LDS_XYZ = (size_t)(2 * PM * XS + PM * ZS) * sizeof(float);
constexpr size_t RO_LDS_DRAWS = (size_t)PM * (PN + 4) * sizeof(float);      // a step's normals and the draw's key

struct RoLds {
    float *X, *Y, *Z;        // [32][XS], [32][XS], [32][ZS]
    float *rest;             // what the unit keeps behind them (the floats before it are a multiple of 8 bytes)
};
__device__ __forceinline__ RoLds ro_carve(float *lds) { return {lds, lds + PM * XS, lds + 2 * PM * XS, lds + 2 * PM * XS + PM * ZS}; }

// What a layer does with its outputs.  The first two are the engine's: ELU into X or Y (rows XS apart), the plain value into Z
// (rows ZS apart: mode `mean`, the prior's mean is the new stoch).  From RO_OUT on the unit's own epilogue is called.
enum { RO_ELU = 0, RO_STORE_Z = 1, RO_OUT = 2 };

struct RoLayer {
    const float *a;          // LDS input, first column; rows `as` apart
    int k;
    const float *a2;         // second part of the input (weight rows k ..), or k2 = 0
    int k2, as;
    const float *w, *b;
    int ld, n;
    float *d;                // LDS output, first column; null where the output leaves the CU
    int kind;
    float *g;                // a head's one column: the caller's array it leaves the CU for, or null (kept apart from d: one pointer
                             // for LDS and global memory would make every epilogue store a flat one)
};

// ---- the recurring shapes
// a head's or the actor's first layer: the feature [stoch 30, deter 200] from the latent, 400 columns -> X
__device__ __forceinline__ RoLayer ro_first(const float *Z, const float *w, const float *b, float *X) {
    return {Z + Z_STOCH, RC_POLICY_STOCH, Z, RC_POLICY_DETER, ZS, w, b, RC_POLICY_LD400, RC_POLICY_UNITS, X, RO_ELU, nullptr};
}
__device__ __forceinline__ RoLayer ro_hidden(const float *src, const float *w, const float *b, float *dst) {
    return {src, RC_POLICY_UNITS, nullptr, 0, XS, w, b, RC_POLICY_LD400, RC_POLICY_UNITS, dst, RO_ELU, nullptr};
}
// a head's one output column: `kind` names it to the unit's epilogue, which knows how `out` (the caller's array, or null) is laid out
__device__ __forceinline__ RoLayer ro_column(const float *src, const float *w, const float *b, int kind, float *out) {
    return {src, RC_POLICY_UNITS, nullptr, 0, XS, w, b, RC_POLICY_LDSMALL, 1, nullptr, kind, out};
}
// the actor's output behind its four hidden layers: 2 columns Y -> Z.action (the sampled modes: as a pair layer on their own image)
template <bool SAMPLED>
__device__ __forceinline__ RoLayer ro_actor_out(const float *Y, const RcPolicyDev &w, const RcPolicySampleDev &ws, float *Z, int kind) {
    return {Y, RC_POLICY_UNITS, nullptr, 0, XS, SAMPLED ? ws.hout_w : w.hout_w, SAMPLED ? ws.hout_b : w.hout_b,
            SAMPLED ? RC_POLICY_LDPAIR : RC_POLICY_LDSMALL, 2, Z + Z_ACTION, kind, nullptr};
}
// the prior: img1 on [stoch, action] (the 32 columns of Z from Z_STOCH), img2 on the new deter, img3 -> stoch (`kind`: RO_STORE_Z
// in mode `mean`; the sampled modes run it as a pair layer)
__device__ __forceinline__ RoLayer ro_img1(const float *Z, const RcPolicyDev &w, float *X) {
    return {Z + Z_STOCH, 32, nullptr, 0, ZS, w.img1_w, w.img1_b, RC_POLICY_LD200, RC_POLICY_DETER, X, RO_ELU, nullptr};
}
__device__ __forceinline__ RoLayer ro_img2(const float *Y, const RcImagineDev &wi, float *X) {
    return {Y, RC_POLICY_DETER, nullptr, 0, XS, wi.img2_w, wi.img2_b, RC_POLICY_LD200, RC_POLICY_DETER, X, RO_ELU, nullptr};
}
__device__ __forceinline__ RoLayer ro_img3(const float *X, const RcImagineDev &wi, float *Z, int kind = RO_STORE_Z) {
    return {X, RC_POLICY_DETER, nullptr, 0, XS, wi.img3_w, wi.img3_b, RC_POLICY_LDPAIR, RC_POLICY_STOCH, Z + Z_STOCH, kind, nullptr};
}

// One wave's 32-column tiles col0, col0 + 128, ... of a layer, k ascending over the input's one or two parts.
// out(L, row, j, v): the unit's epilogue for kinds from RO_OUT on; only layers of one tile have one.
template <int TN, class Out>
__device__ __forceinline__ void ro_dense(const RoLayer &L, int col0, int lane, Out &&out) {
    const int cc = lane & 31, half = lane >> 5;
    int col[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) col[i] = col0 + 128 * i;
    pm_f32x16 acc[TN];
    pm_bias<TN>(acc, L.b, col, cc);
    pm_gemm<TN>(acc, L.a + cc * L.as + half, L.k / 2, L.w + (size_t)half * L.ld + cc, L.ld, col);
    if (L.k2) pm_gemm<TN>(acc, L.a2 + cc * L.as + half, L.k2 / 2, L.w + (size_t)(L.k + half) * L.ld + cc, L.ld, col);
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int j = col[i] + cc;
        if (j >= L.n) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = pm_row(r, half);
            const float v = acc[i][r];
            if (L.kind == RO_ELU) L.d[row * XS + j] = pm_elu(v);
            else if (L.kind == RO_STORE_Z) L.d[row * ZS + j] = v;
            else if constexpr (TN == 1) out(L, row, j, v);
        }
    }
}

// The ladder: wave w of four owns tiles w, w + 4, ... of the layer
template <class Out>
__device__ __forceinline__ void ro_layer(const RoLayer &L, int wave, int lane, Out &&out) {
    const int n_tiles = (L.n + 31) / 32;
    const int mine = wave < n_tiles ? (n_tiles - wave + 3) / 4 : 0;
    if (mine == 1) ro_dense<1>(L, 32 * wave, lane, out);
    else if (mine == 2) ro_dense<2>(L, 32 * wave, lane, out);
    else if (mine == 3) ro_dense<3>(L, 32 * wave, lane, out);
    else if (mine == 4) ro_dense<4>(L, 32 * wave, lane, out);
}

// A pair layer on one wave (the sampled modes' img3 and hout, observe's img3 and obs2 in both modes): the mean columns in tile 0,
// the raw std columns in tile 1 of an ld-64 image, so a (row, column)'s two values sit in matching registers.
// pair(row, j, mean, raw): the unit's epilogue.
template <class Pair>
__device__ __forceinline__ void ro_dense_pair(const RoLayer &L, int lane, Pair &&pair) {
    const int cc = lane & 31, half = lane >> 5;
    const int col[2] = {0, 32};
    pm_f32x16 acc[2];
    pm_bias<2>(acc, L.b, col, cc);
    pm_gemm<2>(acc, L.a + cc * L.as + half, L.k / 2, L.w + (size_t)half * L.ld + cc, L.ld, col);
    if (cc >= L.n) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) pair(pm_row(r, half), cc, acc[0][r], acc[1][r]);
}

// the sampled stoch: mean + (softplus(raw) + 0.1) n
__device__ __forceinline__ float ro_sampled_stoch(float mean, float raw, float n) { return fmaf(pm_softplus(raw) + PM_STOCH_MIN_STD, n, mean); }

// GRU on x = X[0, 200) and h = Z[0, 200), as rc_policy_kernel's: the new deter goes to Y[0, 200) because the other waves still
// read the old one.  (racecar_dream_grad.hip's dg_gru is a copy of this loop that also stores the gates: change both.)
__device__ __forceinline__ void ro_gru(const RcPolicyDev &w, const float *X, const float *Z, float *Y, int wave, int lane) {
    const int cc = lane & 31, half = lane >> 5;
#pragma unroll 1
    for (int jt = wave; jt < RC_POLICY_LD200 / 32; jt += 4) {
        const int col[3] = {32 * jt, RC_POLICY_LD200 + 32 * jt, 2 * RC_POLICY_LD200 + 32 * jt};
        pm_f32x16 mx[3], mh[3];
        pm_bias<3>(mx, w.gru_b, col, cc);
        pm_gemm<3>(mx, X + cc * XS + half, RC_POLICY_DETER / 2, w.gru_k + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
        pm_bias<3>(mh, w.gru_b + RC_POLICY_LDGRU, col, cc);
        pm_gemm<3>(mh, Z + cc * ZS + half, RC_POLICY_DETER / 2, w.gru_r + (size_t)half * RC_POLICY_LDGRU + cc, RC_POLICY_LDGRU, col);
        const int j = 32 * jt + cc;
        if (j < RC_POLICY_DETER) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = pm_row(r, half);
                Y[row * XS + j] = pm_gru(mx[0][r], mx[1][r], mx[2][r], mh[0][r], mh[1][r], mh[2][r], Z[row * ZS + j]);
            }
        }
    }
}

// the new deter into the latent: the GRU's readers of the old one are through (a barrier), nothing reads Z in this phase
__device__ __forceinline__ void ro_commit_deter(const float *Y, float *Z, int tid) {
    for (int idx = tid; idx < PM * RC_POLICY_DETER; idx += PT) {
        const int row = idx / RC_POLICY_DETER, j = idx - row * RC_POLICY_DETER;
        Z[row * ZS + j] = Y[row * XS + j];
    }
}

// ---- per-row staging.  at(row) is the row's index (int64) in the array at hand, -1 where the row has none.
// The latent of the rows: stoch | deter of state row at(row) (the two action columns are not read); zeros where at(row) < 0
template <class At>
__device__ __forceinline__ void ro_load_latent_rows(const float *state, At &&at, float *Z, int tid) {
    for (int idx = tid; idx < PM * ZS; idx += PT) {
        const int row = idx / ZS, j = idx - row * ZS;
        const int64_t l = at(row);
        float v = 0.0f;
        if (l >= 0 && j < FEAT) v = state[(size_t)l * RC_POLICY_STATE + (j < RC_POLICY_DETER ? RC_POLICY_STOCH + j : j - RC_POLICY_DETER)];
        Z[idx] = v;
    }
}

// A step's normals [32][PN]: thread (row, block) = (tid / 8, tid % 8) draws block `block` of its row, the thread of block 0 also
// the action's block where the actor runs.  draw(row, block, out[4]); rows that valid(row) refuses get zeros.
template <class Valid, class Draw>
__device__ __forceinline__ void ro_stage_normals(float *normals, Valid &&valid, Draw &&draw, bool with_action_block, int tid) {
    const int row = tid >> 3, blk = tid & 7;
    const bool action = blk == 0 && with_action_block;
    float n[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid(row)) {
        draw(row, (uint32_t)blk, n);
        if (action) draw(row, (uint32_t)PM_BLOCK_ACTION, m);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        normals[row * PN + 4 * blk + i] = n[i];
        if (action) normals[row * PN + 32 + i] = m[i];
    }
}

// Open loop: the step's given actions [..][2] at at(row), clamped, into the latent, and into `echo` where the caller wants them back
template <class At>
__device__ __forceinline__ void ro_stage_actions(const float *actions_in, float *echo, At &&at, float *Z, int tid) {
    if (tid >= 2 * PM) return;
    const int row = tid >> 1, j = tid & 1;
    const int64_t q = at(row);
    const float a = q >= 0 ? pm_clamp_action(actions_in[(size_t)q * 2 + j]) : 0.0f;
    Z[row * ZS + Z_ACTION + j] = a;
    if (q >= 0 && echo) echo[(size_t)q * 2 + j] = a;
}

// feature = [stoch', deter'] from the latent into dst[at(row)][230] (the latent's next writer is a barrier away)
template <class At>
__device__ __forceinline__ void ro_store_features(float *dst, At &&at, const float *Z, int tid) {
    for (int idx = tid; idx < PM * FEAT; idx += PT) {
        const int row = idx / FEAT, j = idx - row * FEAT;
        const int64_t q = at(row);
        if (q >= 0) dst[(size_t)q * FEAT + j] = Z[row * ZS + (j < RC_POLICY_STOCH ? Z_STOCH + j : j - RC_POLICY_STOCH)];
    }
}

// ---- host: the dynamic-LDS limit of a unit's two kernels, and the launch of the one the call's mode names
template <class Kernel>
hipError_t ro_prepare(Kernel mean, Kernel sampled, size_t bytes, size_t bytes_sampled) {
    const hipError_t e = hipFuncSetAttribute((const void *)mean, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)sampled, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes_sampled);
}

template <class Call>
hipError_t ro_launch(void (*kernel)(Call), int64_t rows, size_t lds_bytes, const Call &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    hipExtLaunchKernelGGL(kernel, dim3((unsigned)((rows + PM - 1) / PM)), dim3(PT), (uint32_t)lds_bytes, s, start, stop, 0u, c);
    return hipGetLastError();
}

}  // namespace
