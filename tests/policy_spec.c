/* The binary32 specification of the deterministic Dreamer agent, restated for the CPU: plain C11, one IEEE
 * operation per written operator, fmaf where a fused operation is meant.  Build: cc -O2 -ffp-contract=off -fno-fast-math
 * (tests/policy_spec.py).  It restates racing_dreamer_amd/csrc/racecar_policy_math.h and the k-ordered fmaf chains of
 * racecar_policy.hip; it includes neither. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PS_STOCH 30
#define PS_DETER 200
#define PS_STATE 232
#define PS_UNITS 400
#define PS_BEAMS 1080

static float ps_exp_parts(float x, float *n_out, float *scale_out) {
    x = x > -86.0f ? x : -86.0f;
    x = x < 86.0f ? x : 86.0f;
    const float n = rintf(x * 0x1.715476p+0f);
    float r = fmaf(n, -0x1.62e400p-1f, x);
    r = fmaf(n, -0x1.7f7d1cp-20f, r);
    float t = fmaf(r, 0.0001984127f, 0.0013888889f);
    t = fmaf(r, t, 0.0083333338f);
    t = fmaf(r, t, 0.041666668f);
    t = fmaf(r, t, 0.16666667f);
    t = fmaf(r, t, 0.5f);
    const float rr = r * r;
    const uint32_t bits = (uint32_t)((int32_t)n + 127) << 23;
    *n_out = n;
    memcpy(scale_out, &bits, 4);
    return fmaf(rr, t, r);
}

float ps_exp(float x) {
    float n, scale;
    const float q = ps_exp_parts(x, &n, &scale);
    return (1.0f + q) * scale;
}

float ps_expm1(float x) {
    float n, scale;
    const float q = ps_exp_parts(x, &n, &scale);
    return n == 0.0f ? q : (1.0f + q) * scale - 1.0f;
}

float ps_elu(float x) { return x > 0.0f ? x : ps_expm1(x); }

float ps_sigmoid(float x) { return 1.0f / (1.0f + ps_exp(-x)); }

float ps_tanh(float x) {
    const float e = ps_expm1(2.0f * fabsf(x));
    return copysignf(e / (e + 2.0f), x);
}

static float ps_preprocess(float scan_m) {
    float c = scan_m > 0.0f ? scan_m : 0.0f;
    c = c < 15.0f ? c : 15.0f;
    return c / 15.0f - 0.5f;
}

float ps_postprocess(float a, float lo, float hi) {
    a = a > -1.0f ? a : -1.0f;
    a = a < 1.0f ? a : 1.0f;
    return ((a + 1.0f) * 0.5f) * (hi - lo) + lo;
}

/* the checkpoint's arrays, row-major as stored */
typedef struct ps_weights {
    const float *gru_kernel, *gru_recurrent, *gru_bias, *img1_w, *img1_b, *obs1_w, *obs1_b, *obs2_w, *obs2_b;
    const float *h_w[4], *h_b[4], *hout_w, *hout_b;
    const float *hnorm_mean, *hnorm_var, *hnorm_gamma, *hnorm_beta;     /* NULL: the plain actor */
} ps_weights;

/* out[j] = bias[j], then for k ascending out[j] = fmaf(x[k], w[k][col0 + j], out[j]): one chain per output, j = 0 .. n - 1 */
static void ps_dense(const float *x, int k_n, const float *w, int ld, int col0, const float *bias, int n, float *out) {
    for (int j = 0; j < n; ++j) out[j] = bias[col0 + j];
    for (int k = 0; k < k_n; ++k) {
        const float xk = x[k];
        const float *row = w + (size_t)k * ld + col0;
        for (int j = 0; j < n; ++j) out[j] = fmaf(xk, row[j], out[j]);
    }
}

/* the dense chain alone over `rows` inputs x [rows][k_n] -> out [rows][n] (w [k_n][n], bias [n]): what tests/test_policy_edge_spec.py
 * holds against exact rational arithmetic with one rounding per fmaf */
void ps_dense_rows(int rows, int k_n, int n, const float *x, const float *w, const float *bias, float *out) {
    for (int i = 0; i < rows; ++i) ps_dense(x + (size_t)i * k_n, k_n, w, n, 0, bias, n, out + (size_t)i * n);
}

/* one agent step for cars [0, n): scan [n][1080] metres, state [n][232] in place, fresh [n] or NULL, action [n][2] raw */
void ps_act(const ps_weights *w, int n, const float *scan, float *state, const uint8_t *fresh, float *action) {
    for (int i = 0; i < n; ++i) {
        float *st = state + (size_t)i * PS_STATE;
        float in1[32], x[PS_DETER], mx[600], mh[600], feat[PS_DETER + PS_BEAMS], a[PS_UNITS], b[PS_UNITS], out[2];
        if (fresh && fresh[i]) memset(st, 0, PS_STATE * sizeof(float));
        memcpy(in1, st, PS_STOCH * sizeof(float));                       /* [stoch, previous action] */
        in1[30] = st[230];
        in1[31] = st[231];
        ps_dense(in1, 32, w->img1_w, 200, 0, w->img1_b, 200, x);
        for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
        const float *h = st + PS_STOCH;
        ps_dense(x, 200, w->gru_kernel, 600, 0, w->gru_bias, 600, mx);
        ps_dense(h, 200, w->gru_recurrent, 600, 0, w->gru_bias + 600, 600, mh);
        for (int j = 0; j < 200; ++j) {                                  /* reset_after: gates z, r, candidate */
            const float z = ps_sigmoid(mx[j] + mh[j]);
            const float r = ps_sigmoid(mx[200 + j] + mh[200 + j]);
            const float cand = ps_tanh(mx[400 + j] + r * mh[400 + j]);
            feat[j] = z * h[j] + (1.0f - z) * cand;
        }
        for (int k = 0; k < PS_BEAMS; ++k) feat[PS_DETER + k] = ps_preprocess(scan[(size_t)i * PS_BEAMS + k]);
        ps_dense(feat, PS_DETER + PS_BEAMS, w->obs1_w, 200, 0, w->obs1_b, 200, x);       /* [deter, embed] */
        for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
        ps_dense(x, 200, w->obs2_w, 60, 0, w->obs2_b, PS_STOCH, a);                      /* the 30 mean columns */
        memcpy(st, a, PS_STOCH * sizeof(float));
        memcpy(st + PS_STOCH, feat, PS_DETER * sizeof(float));
        ps_dense(st, 230, w->h_w[0], 400, 0, w->h_b[0], 400, a);                         /* [stoch, deter] */
        for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
        for (int l = 1; l < 4; ++l) {
            ps_dense(a, 400, w->h_w[l], 400, 0, w->h_b[l], 400, b);
            for (int j = 0; j < 400; ++j) a[j] = ps_elu(b[j]);
        }
        ps_dense(a, 400, w->hout_w, 4, 0, w->hout_b, 2, out);                            /* the 2 mean columns */
        for (int j = 0; j < 2; ++j) {
            float mu;
            if (w->hnorm_mean) mu = (out[j] - w->hnorm_mean[j]) / sqrtf(w->hnorm_var[j] + 1e-3f) * w->hnorm_gamma[j] + w->hnorm_beta[j];
            else mu = 5.0f * ps_tanh(out[j] / 5.0f);
            action[2 * i + j] = st[230 + j] = ps_tanh(mu);
        }
    }
}

void ps_map(int which, int n, const float *x, float *y) {      /* the scalar functions over an array: 0 exp, 1 elu, 2 sigmoid, 3 tanh */
    for (int i = 0; i < n; ++i) y[i] = which == 0 ? ps_exp(x[i]) : which == 1 ? ps_elu(x[i]) : which == 2 ? ps_sigmoid(x[i]) : ps_tanh(x[i]);
}
