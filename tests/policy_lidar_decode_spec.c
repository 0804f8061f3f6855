/* The binary32 specification of the LiDAR distance decoder (rc_policy_decode_lidar; the reference's
 * LidarDistanceDecoder, dreamer/models.py:424-441), for the CPU under the conventions of policy_spec.c: plain C11, one IEEE
 * operation per written operator, fmaf where a fused operation is meant; built with -ffp-contract=off -fno-fast-math by
 * tests/policy_lidar_decode_spec.py.  It restates racing_dreamer_amd/csrc/racecar_decode_lidar.hip and includes nothing of it;
 * the scalar functions (exp, log, softplus, the scan's preprocessing) are those of policy_spec.c / policy_sample_spec.c.
 *
 * An output of dense1 and dense2 is ONE chain: acc = bias[j], then acc = fmaf(x[k], W[k][j], acc), k ascending.  An output of
 * params is the chain from +0.0f and then `acc + bias[j]`: the bias is added last (a narrow decoder's raw-scale bias is near -30).
 *   dense1  230 -> 256 on [stoch 30 | deter 200], no activation
 *   dense2  256 -> 512, ReLU `acc > 0 ? acc : 0`
 *   params  512 -> 2160, leaky ReLU `v > 0 ? v : 0.2f * v` of v = acc + bias
 *   loc[b] = params[b], scale[b] = softplus(params[1080 + b]), b < 1080, in the model's units scan_m / 15 - 0.5.
 * The log-likelihood against a scan in metres: y = preprocess(scan), z = (y - loc) / scale,
 *   term[b] = ((-0.5f * z) * z - log(scale)) - 0.9189385332f.
 * Its order of summation: the 1080 terms, followed by 8 terms +0.0f, make 34 groups of 32.  Within a group the terms are added in
 * a binary tree over the index (neighbours at distance 1, then 2, 4, 8, 16); the 34 group sums are added in ascending order
 * from +0.0f. */
#include "policy_sample_spec.c"

#define PLS_FEAT 230
#define PLS_H1 256
#define PLS_H2 512
#define PLS_BEAMS 1080
#define PLS_GROUPS 34

typedef struct pls_weights {
    const float *dense1_w, *dense1_b;      /* [230][256], [256] */
    const float *dense2_w, *dense2_b;      /* [256][512], [512] */
    const float *params_w, *params_b;      /* [512][2160], [2160] */
} pls_weights;

static float pls_leaky(float v) { return v > 0.0f ? v : 0.2f * v; }

/* the fixed-order sum of the 1080 terms */
float pls_sum(const float *term) {
    float total = 0.0f;
    for (int g = 0; g < PLS_GROUPS; ++g) {
        float v[32];
        for (int i = 0; i < 32; ++i) v[i] = 32 * g + i < PLS_BEAMS ? term[32 * g + i] : 0.0f;
        for (int m = 1; m < 32; m <<= 1)
            for (int i = 0; i < 32; i += 2 * m) v[i] = v[i] + v[i + m];
        total = total + v[0];
    }
    return total;
}

/* rows [0, n): features [n][230]; scan [n][1080] metres or NULL; mean, std [n][1080], loglik [n], each or NULL (loglik needs scan) */
void pls_decode(const pls_weights *w, int n, const float *features, const float *scan, float *mean, float *std, float *loglik) {
    static _Thread_local float h1[PLS_H1], h2[PLS_H2], out[2 * PLS_BEAMS], term[PLS_BEAMS], zero[2 * PLS_BEAMS];
    for (int i = 0; i < n; ++i) {
        ps_dense(features + (size_t)i * PLS_FEAT, PLS_FEAT, w->dense1_w, PLS_H1, 0, w->dense1_b, PLS_H1, h1);
        ps_dense(h1, PLS_H1, w->dense2_w, PLS_H2, 0, w->dense2_b, PLS_H2, h2);
        for (int j = 0; j < PLS_H2; ++j) h2[j] = h2[j] > 0.0f ? h2[j] : 0.0f;
        ps_dense(h2, PLS_H2, w->params_w, 2 * PLS_BEAMS, 0, zero, 2 * PLS_BEAMS, out);
        for (int j = 0; j < 2 * PLS_BEAMS; ++j) out[j] = out[j] + w->params_b[j];
        for (int b = 0; b < PLS_BEAMS; ++b) {
            const float loc = pls_leaky(out[b]);
            const float sd = pss_softplus(pls_leaky(out[PLS_BEAMS + b]));
            if (mean) mean[(size_t)i * PLS_BEAMS + b] = loc;
            if (std) std[(size_t)i * PLS_BEAMS + b] = sd;
            if (loglik) {
                const float z = (ps_preprocess(scan[(size_t)i * PLS_BEAMS + b]) - loc) / sd;
                term[b] = ((-0.5f * z) * z - pss_log(sd)) - 0.9189385332f;
            }
        }
        if (loglik) loglik[i] = pls_sum(term);
    }
}
