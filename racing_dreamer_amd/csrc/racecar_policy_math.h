// The scalar arithmetic of the deterministic Dreamer agent: one IEEE binary32 operation per written
// operator, fmaf where a fused operation is meant.  tests/policy_spec.c (item 14: tests/policy_sample_spec.c) restates every line
// of this file for the CPU - it does not include it - and the GPU tests compare the two bit for bit, so nothing here may go through v_exp_f32 or libm's exp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "racecar_device.h"

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
// (racecar_dream_grad.hip's dg_gru restates these four lines with the gates named, to keep them for the backward: change both)
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

// the clip to [-1, 1] of postprocess_action, and of an action given to imagination from outside
__device__ __forceinline__ float pm_clamp_action(float a) {
    a = a > -1.0f ? a : -1.0f;
    return a < 1.0f ? a : 1.0f;
}

// postprocess_action (racing_dreamer.py:53-59) = ReduceActionSpace (dreamer/wrappers.py:128-130), as the dynamics kernel writes it
__device__ __forceinline__ float pm_postprocess(float a, float lo, float hi) {
    return ((pm_clamp_action(a) + 1.0f) * 0.5f) * (hi - lo) + lo;
}

// ---- the sampled modes: tests/policy_sample_spec.c restates what follows
#define PM_LN2 0x1.62e430p-1f              // ln 2 rounded to binary32
#define PM_SQRT2 0x1.6a09e6p+0f
#define PM_L1 3.3333331174e-1f             // cephes logf: log(1 + f) = f - f^2 / 2 + f^3 P(f) on [sqrt(1/2) - 1, sqrt 2 - 1]
#define PM_L2 -2.4999993993e-1f
#define PM_L3 2.0000714765e-1f
#define PM_L4 -1.6668057665e-1f
#define PM_L5 1.4249322787e-1f
#define PM_L6 -1.2420140846e-1f
#define PM_L7 1.1676998740e-1f
#define PM_L8 -1.1514610310e-1f
#define PM_L9 7.0376836292e-2f
#define PM_STOCH_MIN_STD 0.1f              // models.py:66-81 obs_step: std = softplus(raw) + 0.1
#define PM_ACTION_MIN_STD 1e-4f            // models.py:339-364 ActionDecoder: std = softplus(raw + raw_init_std) + 1e-4
#define PM_RAW_INIT_STD 0x1.3f913cp+2f     // log(exp(5) - 1) = 4.993239..., init_std 5.0 (racing_dreamer.py:23-25), rounded to binary32
#define PM_TWO_PI 0x1.921fb6p+2f
#define PM_2P24_INV 0x1p-24f
#define PM_SAMPLE_TAG 4u                   // Philox counter word 3, bits 24-31 (spawn 0, DR 2, track draw 3)
#define PM_BLOCK_ACTION 8u                 // block 8: words 0-1 the single action sample, words 2-3 the exploration noise (imagination: words 0-1 step t's action draw)
#define PM_BLOCK_CANDIDATES 16u            // blocks 16 + i, i < 50: candidates 2 i and 2 i + 1 of the best of 100
#define PM_CANDIDATES 100

// log of a positive normal number: x = 2^e m, m in [sqrt(1/2), sqrt 2), f = m - 1 (exact); e ln 2 recombined as in pm_exp_parts
__device__ __forceinline__ float pm_log(float x) {
    uint32_t b = __float_as_uint(x);
    int32_t e = (int32_t)(b >> 23) - 127;
    b = (b & 0x007fffffu) | 0x3f800000u;
    if (__uint_as_float(b) > PM_SQRT2) { b -= 0x00800000u; e += 1; }
    const float f = __uint_as_float(b) - 1.0f;
    const float en = (float)e;
    float t = fmaf(f, PM_L9, PM_L8);
    t = fmaf(f, t, PM_L7);
    t = fmaf(f, t, PM_L6);
    t = fmaf(f, t, PM_L5);
    t = fmaf(f, t, PM_L4);
    t = fmaf(f, t, PM_L3);
    t = fmaf(f, t, PM_L2);
    t = fmaf(f, t, PM_L1);
    const float z = f * f;
    float y = (f * z) * t;
    y = fmaf(en, PM_LN2_LO, y);
    y = fmaf(-0.5f, z, y);
    return fmaf(en, PM_LN2_HI, f + y);
}

// log(1 + t), 0 <= t <= 1, without the cancellation for small t: with u = fl(1 + t), log(u) t / (u - 1) (u - 1 is exact, and the
// quotient undoes the rounding of the sum); t itself where u = 1
__device__ __forceinline__ float pm_log1p(float t) {
    const float u = 1.0f + t;
    return u == 1.0f ? t : pm_log(u) * (t / (u - 1.0f));
}

// softplus(x) = max(x, 0) + log1p(exp(-|x|)).  Beyond |x| = 86 pm_exp saturates at exp(-86) = 4.5e-38: x itself, or that.
__device__ __forceinline__ float pm_softplus(float x) {
    return (x > 0.0f ? x : 0.0f) + pm_log1p(pm_exp(-fabsf(x)));
}

// Two standard normals from two Philox words (Box-Muller): u1 in (0, 1], u2 in [0, 1), both multiples of 2^-24 (exact);
// |n| <= sqrt(48 ln 2) = 5.77
__device__ __forceinline__ void pm_normal_pair(uint32_t w0, uint32_t w1, float &n0, float &n1) {
    const float u1 = (float)((w0 >> 8) + 1u) * PM_2P24_INV;
    const float u2 = (float)(w1 >> 8) * PM_2P24_INV;
    const float r = rcd::sqrt_rn(-2.0f * pm_log(u1));
    float sn, cs;
    rcd::sincos32(PM_TWO_PI * u2, sn, cs);
    n0 = r * cs;
    n1 = r * sn;
}

// the four normals of the Philox block whose counter is (env, episode, agent step, word): the two streams below
__device__ __forceinline__ void pm_normal_word(uint32_t env, uint32_t episode, uint32_t agent_step, uint32_t word, uint32_t seed_lo,
                                               uint32_t seed_hi, float (&n)[4]) {
    const rcd::u32x4 r = rcd::philox4x32(env, episode, agent_step, word, seed_lo, seed_hi);
    pm_normal_pair(r.x, r.y, n[0], n[1]);
    pm_normal_pair(r.z, r.w, n[2], n[3]);
}

// the four normals of block `block` of a car's draw ("random stream")
__device__ __forceinline__ void pm_normal_block(uint32_t env, uint32_t episode, uint32_t agent_step, uint32_t slot, uint32_t block,
                                                uint32_t seed_lo, uint32_t seed_hi, float (&n)[4]) {
    pm_normal_word(env, episode, agent_step, block | (slot << 8) | (PM_SAMPLE_TAG << 24), seed_lo, seed_hi, n);
}

// one action dimension's term of a candidate's score: the tanh-normal log-density at the pre-tanh u = mu + sd n without the
// terms that are the same for all of a car's candidates (log sd, log sqrt(2 pi)); log(1 - tanh(u)^2) = 2 (ln 2 - u - softplus(-2 u))
// (dreamer/tools.py:301-321 SampleDist.mode through tfd.TransformedDistribution's tanh bijector)
__device__ __forceinline__ float pm_score_term(float n, float u) {
    const float j = (PM_LN2 - u) - pm_softplus(-2.0f * u);
    return (-0.5f * n) * n - 2.0f * j;
}

// additive_gaussian exploration (models.py:189-202 _exploration) and the clip to +-1 (racing_dreamer.py:53-59)
__device__ __forceinline__ float pm_explore(float a, float amount, float n) {
    const float v = fmaf(amount, n, a);
    return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

// the actor's mean and standard deviation from the output layer's columns j and 2 + j: plain (models.py:339-353) and
// "normalized" (:354-364: batch normalisation of all four columns; hn = mean | sqrt(var + eps) | gamma | beta, 4 each)
__device__ __forceinline__ void pm_actor_dist(float out_mean, float out_std, const float *hn, int j, float &mu, float &sd) {
    if (hn) {
        mu = (out_mean - hn[j]) / hn[4 + j] * hn[8 + j] + hn[12 + j];
        sd = pm_softplus((out_std - hn[2 + j]) / hn[6 + j] * hn[10 + j] + hn[14 + j]) + PM_ACTION_MIN_STD;
    } else {
        mu = 5.0f * pm_tanh(out_mean / 5.0f);
        sd = pm_softplus(out_std + PM_RAW_INIT_STD) + PM_ACTION_MIN_STD;
    }
}

// ---- imagination: tests/policy_imagine_spec.c restates what follows
#define PM_IMAGINE_TAG 5u                  // Philox counter word 3, bits 24-31

// the four normals of block `block` of imagined step t of a car's rollout: blocks 0-7 the prior's 30 normals, PM_BLOCK_ACTION the action draw
__device__ __forceinline__ void pm_imagine_normal_block(uint32_t env, uint32_t episode, uint32_t agent_step, uint32_t slot, uint32_t t,
                                                        uint32_t block, uint32_t seed_lo, uint32_t seed_hi, float (&n)[4]) {
    pm_normal_word(env, episode, agent_step, block | (slot << 8) | (t << 12) | (PM_IMAGINE_TAG << 24), seed_lo, seed_hi, n);
}

// ---- planning in the latent: tests/policy_dream_spec.c restates what follows
#define PM_DREAM_TAG 7u                    // Philox counter word 3, bits 24-31

// the four normals of block `block` (0-7: the 30 normals of stoch', 2 unused) of step t of candidate `cand` of the start with the
// 64-bit id (id_lo, id_hi): t < 64 sits in bits 8-13 of word 3
__device__ __forceinline__ void pm_dream_normal_block(uint32_t id_lo, uint32_t id_hi, uint32_t cand, uint32_t t, uint32_t block,
                                                      uint32_t seed_lo, uint32_t seed_hi, float (&n)[4]) {
    pm_normal_word(id_lo, id_hi, cand, block | (t << 8) | (PM_DREAM_TAG << 24), seed_lo, seed_hi, n);
}

// ---- lambda-returns from given states: tests/policy_returns_spec.c restates what follows
#define PM_RETURNS_TAG 8u                  // Philox counter word 3, bits 24-31

// the four normals of block `block` (0-7: the 30 normals of stoch', 2 unused; PM_BLOCK_ACTION: words 0-1 the action draw) of
// imagined step t of the start with the 64-bit id (id_lo, id_hi)
__device__ __forceinline__ void pm_returns_normal_block(uint32_t id_lo, uint32_t id_hi, uint32_t t, uint32_t block, uint32_t seed_lo,
                                                        uint32_t seed_hi, float (&n)[4]) {
    pm_normal_word(id_lo, id_hi, t, block | (PM_RETURNS_TAG << 24), seed_lo, seed_hi, n);
}

// ---- the LiDAR distance decoder: tests/policy_lidar_decode_spec.c restates its use
#define PM_HALF_LOG_2PI 0.9189385332f      // log(2 pi) / 2 rounded to binary32: the constant of a normal's log-density

// ---- recorded sequences: tests/policy_observe_spec.c restates what follows
#define PM_OBSERVE_TAG 6u                  // Philox counter word 3, bits 24-31

// the four normals of block `block` (0-7: the 30 normals of stoch', 2 unused) of step t of the row with the 64-bit id (row_lo, row_hi)
__device__ __forceinline__ void pm_observe_normal_block(uint32_t row_lo, uint32_t row_hi, uint32_t t, uint32_t block, uint32_t seed_lo,
                                                        uint32_t seed_hi, float (&n)[4]) {
    pm_normal_word(row_lo, row_hi, t, block | (PM_OBSERVE_TAG << 24), seed_lo, seed_hi, n);
}

// one dimension of KL(post || prior) of two diagonal normals (dreamer/models.py:84-110 `_train`, tfd.kl_divergence):
// log sq - log sp + (sp^2 + (mp - mq)^2) / (2 sq^2) - 1/2, p = post, q = prior
__device__ __forceinline__ float pm_kl_term(float mp, float sp, float mq, float sq) {
    const float d = mp - mq;
    const float num = fmaf(d, d, sp * sp);
    const float den = 2.0f * (sq * sq);
    return ((pm_log(sq) - pm_log(sp)) + num / den) - 0.5f;
}
