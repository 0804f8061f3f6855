// The MFMA machinery the Dreamer kernels share (racecar_policy.hip: the agent; racecar_fit.hip and racecar_decode.hip; through
// racecar_rollout.h the four rollout units): one workgroup of four waves owns 32 cars = the rows of v_mfma_f32_32x32x2_f32 tiles;
// activations lie in LDS rows of an odd stride, weights are read from L2 straight into the B operand.  Below the k loop (pm_gemm):
// the row-to-car map of a call and the packing of the stored latent into LDS.  The dense wrapper, the tile ladder and the GRU loop
// of the rollout units are in racecar_rollout.h; the agent and the fit keep their own (DESIGN.md §4 says why).
// Not part of the public interface.
#pragma once
#include "racecar_policy.h"
#include "racecar_policy_math.h"

typedef float pm_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int PT = 256;                        // threads per workgroup
constexpr int PM = RC_POLICY_TILE;             // cars per workgroup
constexpr int XS = 417;                        // row stride of X and Y [floats]
constexpr int PD = 4;                          // k-steps (of 2) whose operands are requested one block ahead
constexpr int PN = 36;                         // normals per car and draw: blocks 0-7 (the 30 of stoch, 2 unused), the 4 of block 8

// acc[t] += A[32 x 2 ksteps] W[2 ksteps x 32 columns at col[t]], k ascending.  a = &A[lane & 31][lane >> 5] (LDS),
// w = &W[lane >> 5][lane & 31] (global).  The operands of the next PD k-steps are requested before this block's MFMAs issue;
// past the end the last step is requested again (a valid address) and not used.
template <int TN>
__device__ __forceinline__ void pm_gemm(pm_f32x16 (&acc)[TN], const float *a, int ksteps, const float *__restrict__ w, int ld,
                                        const int (&col)[TN]) {
    float ac[PD], bc[PD][TN], an[PD], bn[PD][TN];
#pragma unroll
    for (int u = 0; u < PD; ++u) {
        const int s = u < ksteps ? u : ksteps - 1;
        ac[u] = a[2 * s];
#pragma unroll
        for (int t = 0; t < TN; ++t) bc[u][t] = w[(size_t)(2 * s) * ld + col[t]];
    }
#pragma unroll 1
    for (int s0 = 0; s0 < ksteps; s0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            int s = s0 + PD + u;
            s = s < ksteps ? s : ksteps - 1;
            an[u] = a[2 * s];
#pragma unroll
            for (int t = 0; t < TN; ++t) bn[u][t] = w[(size_t)(2 * s) * ld + col[t]];
        }
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            if (s0 + u < ksteps) {
#pragma unroll
                for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u], bc[u][t], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            ac[u] = an[u];
#pragma unroll
            for (int t = 0; t < TN; ++t) bc[u][t] = bn[u][t];
        }
    }
}

template <int TN>
__device__ __forceinline__ void pm_bias(pm_f32x16 (&acc)[TN], const float *__restrict__ b, const int (&col)[TN], int c) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const float v = b[col[t] + c];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = v;
    }
}

// C/D map of the 32x32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int pm_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// row q of the call -> car index (the mask's slots of env q / n_slots), -1 past the end
__device__ __forceinline__ int pm_car(const RcPolicyRows &c, int q) {
    if (q >= c.n_active) return -1;
    const int e = q / c.n_slots, k = q - e * c.n_slots;
    return e * c.cars_per_env + (int)((c.slots >> (8 * k)) & 0xffu);
}

// The stored latent of the workgroup's rows into LDS, dst rows ds apart: deter at [0, 200), stoch at [200, 230), the previous raw
// action at [230, 232); zero for rows past the end and wherever keep(car, column of the state) says no
template <class Keep>
__device__ __forceinline__ void pm_load_latent(const RcPolicyRows &c, const float *state, float *dst, int ds, int row0, int tid, Keep &&keep) {
    for (int idx = tid; idx < PM * RC_POLICY_STATE; idx += PT) {
        const int row = idx / RC_POLICY_STATE, j = idx - row * RC_POLICY_STATE;
        const int car = pm_car(c, row0 + row);
        const float v = car >= 0 && keep(car, j) ? state[(size_t)car * RC_POLICY_STATE + j] : 0.0f;
        int at;
        if (j < RC_POLICY_STOCH) at = RC_POLICY_DETER + j;
        else if (j < RC_POLICY_STOCH + RC_POLICY_DETER) at = j - RC_POLICY_STOCH;
        else at = j;                                                // (the action's 2 columns follow stoch's 30)
        dst[row * ds + at] = v;
    }
}

}  // namespace
