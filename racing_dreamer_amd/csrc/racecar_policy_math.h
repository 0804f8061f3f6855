// The scalar arithmetic of the deterministic Dreamer agent: one IEEE binary32 operation per written
// operator, fmaf where a fused operation is meant.  tests/policy_spec.c restates every line of this file for the CPU - it does
// not include it - and the GPU tests compare the two bit for bit, so nothing here may go through v_exp_f32 or libm's exp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PM_EXP_CLAMP 86.0f                 // exp's argument is clamped to +-86: 2^n stays a normal number for every n = rint(x log2 e)
#define PM_LOG2E 0x1.715476p+0f            // log2(e) rounded to binary32
#define PM_LN2_HI 0x1.62e400p-1f           // ln 2 = HI + LO, HI with 9 trailing zero bits: n * HI is exact for |n| < 512
#define PM_LN2_LO 0x1.7f7d1cp-20f
#define PM_C2 0.5f                         // Taylor coefficients of (exp(r) - 1 - r) / r^2, |r| <= ln 2 / 2: the first dropped
#define PM_C3 0.16666667f                  // term, r^8 / 8!, is below 2^-26 of the result
#define PM_C4 0.041666668f
#define PM_C5 0.0083333338f
#define PM_C6 0.0013888889f
#define PM_C7 0.0001984127f
#define PM_SCAN_MAX 15.0f                  // racing_dreamer.py:44-52 _preprocess_lidar: clip to [0, 15] m, / 15, - 0.5
#define PM_BN_EPS 1e-3f                    // Keras BatchNormalization epsilon

// exp(x) = 2^n (1 + q): n = rint(x log2 e), r = x - n ln 2 in two fused steps, q = r + r^2 P(r).  Returns q, n and 2^n.
__device__ __forceinline__ float pm_exp_parts(float x, float *n_out, float *scale_out) {
    x = x > -PM_EXP_CLAMP ? x : -PM_EXP_CLAMP;
    x = x < PM_EXP_CLAMP ? x : PM_EXP_CLAMP;
    const float n = rintf(x * PM_LOG2E);
    float r = fmaf(n, -PM_LN2_HI, x);
    r = fmaf(n, -PM_LN2_LO, r);
    float t = fmaf(r, PM_C7, PM_C6);
    t = fmaf(r, t, PM_C5);
    t = fmaf(r, t, PM_C4);
    t = fmaf(r, t, PM_C3);
    t = fmaf(r, t, PM_C2);
    const float rr = r * r;
    *n_out = n;
    *scale_out = __uint_as_float((uint32_t)((int32_t)n + 127) << 23);       // ldexp(1, n), n in [-124, 124]
    return fmaf(rr, t, r);
}

__device__ __forceinline__ float pm_exp(float x) {
    float n, scale;
    const float q = pm_exp_parts(x, &n, &scale);
    return (1.0f + q) * scale;
}

// exp(x) - 1 without the cancellation near 0: for n = 0 it is q itself
__device__ __forceinline__ float pm_expm1(float x) {
    float n, scale;
    const float q = pm_exp_parts(x, &n, &scale);
    return n == 0.0f ? q : (1.0f + q) * scale - 1.0f;
}

__device__ __forceinline__ float pm_elu(float x) { return x > 0.0f ? x : pm_expm1(x); }

__device__ __forceinline__ float pm_sigmoid(float x) { return 1.0f / (1.0f + pm_exp(-x)); }

// tanh |x| = e / (e + 2) with e = exp(2 |x|) - 1
__device__ __forceinline__ float pm_tanh(float x) {
    const float e = pm_expm1(2.0f * fabsf(x));
    return copysignf(e / (e + 2.0f), x);
}

__device__ __forceinline__ float pm_preprocess(float scan_m) {
    float c = scan_m > 0.0f ? scan_m : 0.0f;
    c = c < PM_SCAN_MAX ? c : PM_SCAN_MAX;
    return c / PM_SCAN_MAX - 0.5f;
}

// tf.keras GRUCell, reset_after = True (models.py:61-87 through the cell): gates from the two matmuls' z, r and candidate columns
__device__ __forceinline__ float pm_gru(float xz, float xr, float xh, float hz, float hr, float hh, float h) {
    const float z = pm_sigmoid(xz + hz);
    const float r = pm_sigmoid(xr + hr);
    const float cand = pm_tanh(xh + r * hh);
    return z * h + (1.0f - z) * cand;
}

// ActionDecoder 'tanh_normal' (models.py:339-353): mean 5 tanh(out / 5); the deterministic agent's command is tanh(mean)
__device__ __forceinline__ float pm_action_plain(float out) { return pm_tanh(5.0f * pm_tanh(out / 5.0f)); }

// actor_version "normalized" (models.py:354-364): inference-mode batch normalisation of the output layer, linear mean
// (sd = sqrtf(var + PM_BN_EPS), an IEEE square root of two weights: taken once when the weights are loaded, on the host)
__device__ __forceinline__ float pm_action_normalized(float out, float mean, float sd, float gamma, float beta) {
    return pm_tanh((out - mean) / sd * gamma + beta);
}

// postprocess_action (racing_dreamer.py:53-59) = ReduceActionSpace (dreamer/wrappers.py:128-130), as the dynamics kernel writes it
__device__ __forceinline__ float pm_postprocess(float a, float lo, float hi) {
    a = a > -1.0f ? a : -1.0f;
    a = a < 1.0f ? a : 1.0f;
    return ((a + 1.0f) * 0.5f) * (hi - lo) + lo;
}
