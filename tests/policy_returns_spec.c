/* The binary32 specification of the critic and the lambda-return (rc_policy_returns), restated for the CPU
 * under the conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is
 * meant; built with -ffp-contract=off -fno-fast-math by tests/policy_returns_spec.py).  It includes policy_imagine_spec.c - and
 * through it policy_sample_spec.c and policy_spec.c - unchanged for the scalar functions, the dense chains, Philox, the normals
 * and the reward head, and restates the loop of racing_dreamer_amd/csrc/racecar_returns.hip and the part of
 * racecar_policy_math.h that belongs to it; it includes neither.  The arithmetic is the reference's dreamer/models.py:113-133
 * (the three heads on the imagined features) and dreamer/tools.py:396-418 (lambda_return through static_scan(reverse=True)). */
#include "policy_imagine_spec.c"

typedef struct prs_critic {
    const float *vh_w[3], *vh_b[3], *vout_w, *vout_b;          /* the value head, or all NULL */
    const float *ph_w[3], *ph_b[3], *pout_w, *pout_b;          /* the pcont head, or all NULL */
} prs_critic;

/* the four normals of block `block` of imagined step t of the start with the 64-bit id: tag 8 */
void prs_normal_block(uint64_t id, uint32_t t, uint32_t block, uint32_t seed_lo, uint32_t seed_hi, float n[4]) {
    uint32_t r[4];
    pss_philox((uint32_t)id, (uint32_t)(id >> 32), t, block | (8u << 24), seed_lo, seed_hi, r);
    pss_normal_pair(r[0], r[1], &n[0], &n[1]);
    pss_normal_pair(r[2], r[3], &n[2], &n[3]);
}

/* DenseDecoder((), 3, 400) on a feature: the one output column before any distribution */
static float prs_head3(const float *const hw[3], const float *const hb[3], const float *out_w, const float *out_b, const float *feat) {
    float a[PS_UNITS], b[PS_UNITS], r;
    ps_dense(feat, PIS_FEAT, hw[0], 400, 0, hb[0], 400, a);
    for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
    ps_dense(a, 400, hw[1], 400, 0, hb[1], 400, b);
    for (int j = 0; j < 400; ++j) b[j] = ps_elu(b[j]);
    ps_dense(b, 400, hw[2], 400, 0, hb[2], 400, a);
    for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
    ps_dense(a, 400, out_w, 1, 0, out_b, 1, &r);
    return r;
}

/* lambda_return and the cumprod for one row: r, v, p [H] -> ret, weight [H - 1] (either may be NULL) */
void prs_lambda_return(int H, const float *r, const float *v, const float *p, float lambda, float *ret, float *weight) {
    if (ret) {
        float R = v[H - 1];
        for (int t = H - 2; t >= 0; --t) {
            const float in = fmaf(p[t] * v[t + 1], 1.0f - lambda, r[t]);
            R = fmaf(p[t] * lambda, R, in);
            ret[t] = R;
        }
    }
    if (weight) {
        float w = 1.0f;
        for (int t = 0; t < H - 1; ++t) {
            weight[t] = w;
            w = w * p[t];
        }
    }
}

/* H imagined steps for rows [0, n) in mode 0 (mean) or 1 (sample) from state [n][232] (stoch | deter | unused), not modified.
 * keyed 0: keys uint32 [n][4], the draws of pis_imagine (live latents); keyed 1: keys uint64 [n], the start ids under tag 8.
 * actions_in [n][H][2] or NULL (the actor's).  Outputs, each optional: reward, value, pcont [n][H], ret, weight [n][H - 1],
 * actions [n][H][2], features [n][H][230], start [3][n] (reward, value, pcont on the starting feature; a head that is not there
 * leaves its row alone), normals [n][H][PIS_NORMALS]. */
void prs_returns(const ps_weights *w, const pis_heads *hd, const prs_critic *cr, int mode, uint32_t seed_lo, uint32_t seed_hi, int n, int H,
                 float lambda, float discount, const float *state, int keyed, const void *keys, const float *actions_in, float *reward,
                 float *value, float *pcont, float *ret, float *weight, float *actions, float *features, float *start, int n_start, float *normals) {
    for (int i = 0; i < n; ++i) {
        float st[PIS_FEAT], rs[64], vs[64], ps[64];
        memcpy(st, state + (size_t)i * PS_STATE, sizeof st);
        const uint32_t *key = keyed ? NULL : (const uint32_t *)keys + 4 * (size_t)i;
        const uint64_t id = keyed ? ((const uint64_t *)keys)[i] : 0;
        if (start) {
            if (hd->rout_w) start[i] = pis_reward(hd, st);
            if (cr->vout_w) start[(size_t)n_start + i] = prs_head3(cr->vh_w, cr->vh_b, cr->vout_w, cr->vout_b, st);
            if (cr->pout_w) start[2 * (size_t)n_start + i] = ps_sigmoid(prs_head3(cr->ph_w, cr->ph_b, cr->pout_w, cr->pout_b, st));
        }
        for (int t = 0; t < H; ++t) {
            const size_t it = (size_t)i * H + t;
            float nrm[PIS_NORMALS], in1[32], x[PS_DETER], mx[600], mh[600], a[PS_UNITS], b[PS_UNITS], out[60], deter[PS_DETER];
            memset(nrm, 0, sizeof nrm);
            if (mode == 1) {
                for (uint32_t blk = 0; blk < 9; ++blk) {
                    if (blk == 8 && actions_in) break;
                    if (keyed) prs_normal_block(id, (uint32_t)t, blk, seed_lo, seed_hi, nrm + 4 * blk);
                    else pis_normal_block(key, (uint32_t)t, blk, seed_lo, seed_hi, nrm + 4 * blk);
                }
            }
            if (normals) memcpy(normals + it * PIS_NORMALS, nrm, sizeof nrm);
            float act[2];
            if (actions_in) {
                for (int j = 0; j < 2; ++j) act[j] = pis_clamp(actions_in[2 * it + j]);
            } else {
                ps_dense(st, PIS_FEAT, w->h_w[0], 400, 0, w->h_b[0], 400, a);
                for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
                for (int l = 1; l < 4; ++l) {
                    ps_dense(a, 400, w->h_w[l], 400, 0, w->h_b[l], 400, b);
                    for (int j = 0; j < 400; ++j) a[j] = ps_elu(b[j]);
                }
                ps_dense(a, 400, w->hout_w, 4, 0, w->hout_b, mode == 1 ? 4 : 2, out);
                for (int j = 0; j < 2; ++j) {
                    float mu, sd = 0.0f;
                    if (w->hnorm_mean) {
                        mu = (out[j] - w->hnorm_mean[j]) / sqrtf(w->hnorm_var[j] + 1e-3f) * w->hnorm_gamma[j] + w->hnorm_beta[j];
                        if (mode == 1)
                            sd = pss_softplus((out[2 + j] - w->hnorm_mean[2 + j]) / sqrtf(w->hnorm_var[2 + j] + 1e-3f) * w->hnorm_gamma[2 + j]
                                              + w->hnorm_beta[2 + j]) + 1e-4f;
                    } else {
                        mu = 5.0f * ps_tanh(out[j] / 5.0f);
                        if (mode == 1) sd = pss_softplus(out[2 + j] + 0x1.3f913cp+2f) + 1e-4f;
                    }
                    act[j] = mode == 1 ? ps_tanh(fmaf(sd, nrm[32 + j], mu)) : ps_tanh(mu);
                }
            }
            if (actions) { actions[2 * it] = act[0]; actions[2 * it + 1] = act[1]; }
            /* img_step: img1 on [stoch, action], the GRU as ps_act's, img2, img3 */
            memcpy(in1, st, PS_STOCH * sizeof(float));
            in1[30] = act[0];
            in1[31] = act[1];
            ps_dense(in1, 32, w->img1_w, 200, 0, w->img1_b, 200, x);
            for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
            const float *h = st + PS_STOCH;
            ps_dense(x, 200, w->gru_kernel, 600, 0, w->gru_bias, 600, mx);
            ps_dense(h, 200, w->gru_recurrent, 600, 0, w->gru_bias + 600, 600, mh);
            for (int j = 0; j < 200; ++j) {
                const float z = ps_sigmoid(mx[j] + mh[j]);
                const float r = ps_sigmoid(mx[200 + j] + mh[200 + j]);
                const float cand = ps_tanh(mx[400 + j] + r * mh[400 + j]);
                deter[j] = z * h[j] + (1.0f - z) * cand;
            }
            ps_dense(deter, 200, hd->img2_w, 200, 0, hd->img2_b, 200, x);
            for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
            ps_dense(x, 200, hd->img3_w, 60, 0, hd->img3_b, mode == 1 ? 60 : PS_STOCH, out);        /* mean | raw std */
            for (int j = 0; j < PS_STOCH; ++j) st[j] = mode == 1 ? fmaf(pss_softplus(out[PS_STOCH + j]) + 0.1f, nrm[j], out[j]) : out[j];
            memcpy(st + PS_STOCH, deter, sizeof deter);
            if (features) memcpy(features + it * PIS_FEAT, st, sizeof st);
            /* the three heads on the new feature: reward(feat).mode(), value(feat).mode(), pcont(feat).mean() or the constant */
            rs[t] = hd->rout_w ? pis_reward(hd, st) : 0.0f;
            vs[t] = cr->vout_w ? prs_head3(cr->vh_w, cr->vh_b, cr->vout_w, cr->vout_b, st) : 0.0f;
            ps[t] = cr->pout_w ? ps_sigmoid(prs_head3(cr->ph_w, cr->ph_b, cr->pout_w, cr->pout_b, st)) : discount;
            if (reward) reward[it] = rs[t];
            if (value) value[it] = vs[t];
            if (pcont) pcont[it] = ps[t];
        }
        if (H >= 2) prs_lambda_return(H, rs, vs, ps, lambda, ret ? ret + (size_t)i * (H - 1) : NULL, weight ? weight + (size_t)i * (H - 1) : NULL);
    }
}

/* 4 n_blocks normals of step t of start `id`: blocks first_block .. (the generator's statistics) */
void prs_normals(uint64_t id, uint32_t t, uint32_t first_block, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, float *out) {
    for (int b = 0; b < n_blocks; ++b) prs_normal_block(id, t, first_block + (uint32_t)b, seed_lo, seed_hi, out + 4 * b);
}
