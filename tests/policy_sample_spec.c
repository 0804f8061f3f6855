/* The binary32 specification of the Dreamer agent's sampled modes, restated for the CPU: the conventions of
 * policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is meant; built with
 * -ffp-contract=off -fno-fast-math by tests/policy_sample_spec.py), which it includes unchanged for the deterministic agent and
 * the scalar functions.  It restates the second half of racing_dreamer_amd/csrc/racecar_policy_math.h, sincos32 and Philox4x32-10
 * of racecar_device.h, and the sampled epilogues of racecar_policy.hip; it includes none of them. */
#include "policy_spec.c"

#define PSS_NORMALS 236          /* per car: 32 of the posterior (30 used), 4 of block 8, 200 of the candidates */

static float pss_from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t pss_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

float pss_log(float x) {
    uint32_t b = pss_bits(x);
    int32_t e = (int32_t)(b >> 23) - 127;
    b = (b & 0x007fffffu) | 0x3f800000u;
    if (pss_from_bits(b) > 0x1.6a09e6p+0f) { b -= 0x00800000u; e += 1; }
    const float f = pss_from_bits(b) - 1.0f;
    const float en = (float)e;
    float t = fmaf(f, 7.0376836292e-2f, -1.1514610310e-1f);
    t = fmaf(f, t, 1.1676998740e-1f);
    t = fmaf(f, t, -1.2420140846e-1f);
    t = fmaf(f, t, 1.4249322787e-1f);
    t = fmaf(f, t, -1.6668057665e-1f);
    t = fmaf(f, t, 2.0000714765e-1f);
    t = fmaf(f, t, -2.4999993993e-1f);
    t = fmaf(f, t, 3.3333331174e-1f);
    const float z = f * f;
    float y = (f * z) * t;
    y = fmaf(en, 0x1.7f7d1cp-20f, y);
    y = fmaf(-0.5f, z, y);
    return fmaf(en, 0x1.62e400p-1f, f + y);
}

static float pss_log1p(float t) {
    const float u = 1.0f + t;
    return u == 1.0f ? t : pss_log(u) * (t / (u - 1.0f));
}

float pss_softplus(float x) { return (x > 0.0f ? x : 0.0f) + pss_log1p(ps_exp(-fabsf(x))); }

static void pss_sincos(float a, float *sn, float *cs) {            /* racecar_device.h sincos32 */
    const float kf = rintf(a * 0.636619772367581343f);
    const float r = ((a - kf * 1.5703125f) - kf * 4.837512969970703125e-4f) - kf * 7.54978995489188216e-8f;
    const int q = ((int)kf) & 3;
    const float z = r * r;
    const float s = r + (r * z) * (-1.6666654611e-1f + z * (8.3321608736e-3f + z * -1.9515295891e-4f));
    const float c = (1.0f - 0.5f * z) + (z * z) * (4.166664568298827e-2f + z * (-1.388731625493765e-3f + z * 2.443315711809948e-5f));
    *sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
    *cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

static void pss_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static void pss_normal_pair(uint32_t w0, uint32_t w1, float *n0, float *n1) {
    const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(w1 >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * pss_log(u1));
    float sn, cs;
    pss_sincos(0x1.921fb6p+2f * u2, &sn, &cs);
    *n0 = r * cs;
    *n1 = r * sn;
}

/* key = (global env, episode, agent step, slot) */
void pss_normal_block(const uint32_t key[4], uint32_t block, uint32_t seed_lo, uint32_t seed_hi, float n[4]) {
    uint32_t r[4];
    pss_philox(key[0], key[1], key[2], block | (key[3] << 8) | (4u << 24), seed_lo, seed_hi, r);
    pss_normal_pair(r[0], r[1], &n[0], &n[1]);
    pss_normal_pair(r[2], r[3], &n[2], &n[3]);
}

static float pss_score_term(float n, float u) {
    const float j = (0x1.62e430p-1f - u) - pss_softplus(-2.0f * u);
    return (-0.5f * n) * n - 2.0f * j;
}

static float pss_explore(float a, float amount, float n) {
    const float v = fmaf(amount, n, a);
    return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

/* One agent step for cars [0, n) in mode 1 (deploy) or 2 (explore); mode 0 is ps_act.  keys [n][4] as above.  Optional outputs:
 * normals [n][PSS_NORMALS] (posterior block b word i at 4 b + i, block 8 at 32, candidate s dimension j at 36 + 2 s + j),
 * winner [n] (deploy: the chosen candidate, else -1), dist [n][4] = mu 0, mu 1, sd 0, sd 1. */
void pss_act(const ps_weights *w, int mode, uint32_t seed_lo, uint32_t seed_hi, float expl_amount, int n, const float *scan, float *state,
             const uint8_t *fresh, const uint32_t *keys, float *action, float *normals, int32_t *winner, float *dist) {
    if (mode == 0) {
        ps_act(w, n, scan, state, fresh, action);
        return;
    }
    for (int i = 0; i < n; ++i) {
        float *st = state + (size_t)i * PS_STATE;
        const uint32_t *key = keys + 4 * (size_t)i;
        float in1[32], x[PS_DETER], mx[600], mh[600], feat[PS_DETER + PS_BEAMS], a[PS_UNITS], b[PS_UNITS], out[4], nrm[PSS_NORMALS];
        for (uint32_t blk = 0; blk < 8; ++blk) pss_normal_block(key, blk, seed_lo, seed_hi, nrm + 4 * blk);
        pss_normal_block(key, 8u, seed_lo, seed_hi, nrm + 32);
        for (uint32_t blk = 0; blk < 50; ++blk) pss_normal_block(key, 16u + blk, seed_lo, seed_hi, nrm + 36 + 4 * blk);
        if (normals) memcpy(normals + (size_t)i * PSS_NORMALS, nrm, sizeof nrm);
        if (fresh && fresh[i]) memset(st, 0, PS_STATE * sizeof(float));
        memcpy(in1, st, PS_STOCH * sizeof(float));
        in1[30] = st[230];
        in1[31] = st[231];
        ps_dense(in1, 32, w->img1_w, 200, 0, w->img1_b, 200, x);
        for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
        const float *h = st + PS_STOCH;
        ps_dense(x, 200, w->gru_kernel, 600, 0, w->gru_bias, 600, mx);
        ps_dense(h, 200, w->gru_recurrent, 600, 0, w->gru_bias + 600, 600, mh);
        for (int j = 0; j < 200; ++j) {
            const float z = ps_sigmoid(mx[j] + mh[j]);
            const float r = ps_sigmoid(mx[200 + j] + mh[200 + j]);
            const float cand = ps_tanh(mx[400 + j] + r * mh[400 + j]);
            feat[j] = z * h[j] + (1.0f - z) * cand;
        }
        for (int k = 0; k < PS_BEAMS; ++k) feat[PS_DETER + k] = ps_preprocess(scan[(size_t)i * PS_BEAMS + k]);
        ps_dense(feat, PS_DETER + PS_BEAMS, w->obs1_w, 200, 0, w->obs1_b, 200, x);
        for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
        ps_dense(x, 200, w->obs2_w, 60, 0, w->obs2_b, 60, a);                            /* mean | raw std */
        for (int j = 0; j < PS_STOCH; ++j) st[j] = fmaf(pss_softplus(a[PS_STOCH + j]) + 0.1f, nrm[j], a[j]);
        memcpy(st + PS_STOCH, feat, PS_DETER * sizeof(float));
        ps_dense(st, 230, w->h_w[0], 400, 0, w->h_b[0], 400, a);
        for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
        for (int l = 1; l < 4; ++l) {
            ps_dense(a, 400, w->h_w[l], 400, 0, w->h_b[l], 400, b);
            for (int j = 0; j < 400; ++j) a[j] = ps_elu(b[j]);
        }
        ps_dense(a, 400, w->hout_w, 4, 0, w->hout_b, 4, out);
        float mu[2], sd[2];
        for (int j = 0; j < 2; ++j) {
            if (w->hnorm_mean) {
                mu[j] = (out[j] - w->hnorm_mean[j]) / sqrtf(w->hnorm_var[j] + 1e-3f) * w->hnorm_gamma[j] + w->hnorm_beta[j];
                sd[j] = pss_softplus((out[2 + j] - w->hnorm_mean[2 + j]) / sqrtf(w->hnorm_var[2 + j] + 1e-3f) * w->hnorm_gamma[2 + j]
                                     + w->hnorm_beta[2 + j]) + 1e-4f;
            } else {
                mu[j] = 5.0f * ps_tanh(out[j] / 5.0f);
                sd[j] = pss_softplus(out[2 + j] + 0x1.3f913cp+2f) + 1e-4f;
            }
        }
        if (dist) { dist[4 * i] = mu[0]; dist[4 * i + 1] = mu[1]; dist[4 * i + 2] = sd[0]; dist[4 * i + 3] = sd[1]; }
        const float *pick = nrm + 32;
        int best_s = -1;
        if (mode == 1) {
            float best = 0.0f;
            for (int s = 0; s < 100; ++s) {
                const float *c = nrm + 36 + 2 * s;
                const float sc = pss_score_term(c[0], fmaf(sd[0], c[0], mu[0])) + pss_score_term(c[1], fmaf(sd[1], c[1], mu[1]));
                if (best_s < 0 || sc > best) { best = sc; best_s = s; }
            }
            pick = nrm + 36 + 2 * best_s;
        }
        if (winner) winner[i] = best_s;
        for (int j = 0; j < 2; ++j)
            action[2 * i + j] = st[230 + j] = pss_explore(ps_tanh(fmaf(sd[j], pick[j], mu[j])), expl_amount, nrm[34 + j]);
    }
}

void pss_map(int which, int n, const float *x, float *y) {      /* 0 log, 1 softplus */
    for (int i = 0; i < n; ++i) y[i] = which == 0 ? pss_log(x[i]) : pss_softplus(x[i]);
}

/* the candidates' scores of one car's distribution, as pss_act computes them (for the test's error bound) */
void pss_scores(const float *dist, const float *cand, float *score) {
    for (int s = 0; s < 100; ++s)
        score[s] = pss_score_term(cand[2 * s], fmaf(dist[2], cand[2 * s], dist[0])) + pss_score_term(cand[2 * s + 1], fmaf(dist[3], cand[2 * s + 1], dist[1]));
}

/* n normals of a fixed key family: block b of key -> out[4 b ..] (the generator's statistics) */
void pss_normals(const uint32_t key[4], uint32_t first_block, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, float *out) {
    for (int b = 0; b < n_blocks; ++b) pss_normal_block(key, first_block + (uint32_t)b, seed_lo, seed_hi, out + 4 * b);
}
