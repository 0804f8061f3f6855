/* The binary32 specification of the world model over recorded sequences (rc_policy_observe), restated for the
 * CPU under the conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is
 * meant; built with -ffp-contract=off -fno-fast-math by tests/policy_observe_spec.py).  It includes policy_imagine_spec.c - and
 * through it policy_sample_spec.c and policy_spec.c - unchanged for the scalar functions, the dense chains, Philox, the normals and
 * the reward head, and restates the loop of racing_dreamer_amd/csrc/racecar_observe.hip and the last part of
 * racecar_policy_math.h; it includes neither. */
#include "policy_imagine_spec.c"

#define POS_NORMALS 32           /* per row and step: blocks 0-7 (30 used) */

/* row_id = row_offset + row, t = the step */
void pos_normal_block(uint64_t row_id, uint32_t t, uint32_t block, uint32_t seed_lo, uint32_t seed_hi, float n[4]) {
    uint32_t r[4];
    pss_philox((uint32_t)row_id, (uint32_t)(row_id >> 32), t, block | (6u << 24), seed_lo, seed_hi, r);
    pss_normal_pair(r[0], r[1], &n[0], &n[1]);
    pss_normal_pair(r[2], r[3], &n[2], &n[3]);
}

/* one dimension of KL(p || q), p = post, q = prior */
static float pos_kl_term(float mp, float sp, float mq, float sq) {
    const float d = mp - mq;
    const float num = fmaf(d, d, sp * sp);
    const float den = 2.0f * (sq * sq);
    return ((pss_log(sq) - pss_log(sp)) + num / den) - 0.5f;
}

/* T steps of rows [0, n) in mode 0 (mean) or 1 (sample): scan [n][T][1080] metres, actions [n][T][2] raw, state_in [n][232] (stoch |
 * deter | not read) or NULL (zeros).  Steps t < context take the posterior's stoch, the others the prior's.  Outputs, each optional:
 * features [n][T][230], post_mean / post_std / prior_mean / prior_std [n][T][30], kl [n][T], reward [n][T] (needs the head),
 * state_out [n][232], normals [n][T][POS_NORMALS]; post_* and kl are written for t < context only. */
void pos_observe(const ps_weights *w, const pis_heads *hd, int mode, uint32_t seed_lo, uint32_t seed_hi, uint64_t row_offset, int n, int T,
                 int context, const float *scan, const float *actions, const float *state_in, float *features, float *post_mean, float *post_std,
                 float *prior_mean, float *prior_std, float *kl, float *reward, float *state_out, float *normals) {
    for (int i = 0; i < n; ++i) {
        float st[PS_STATE];
        memset(st, 0, sizeof st);
        if (state_in) memcpy(st, state_in + (size_t)i * PS_STATE, PIS_FEAT * sizeof(float));
        for (int t = 0; t < T; ++t) {
            const size_t it = (size_t)i * T + t;
            float nrm[POS_NORMALS], in1[32], x[PS_DETER], mx[600], mh[600], out[60], feat[PS_DETER + PS_BEAMS];
            float qm[PS_STOCH], qs[PS_STOCH], pm[PS_STOCH], ps[PS_STOCH];
            memset(nrm, 0, sizeof nrm);
            if (mode == 1)
                for (uint32_t blk = 0; blk < 8; ++blk) pos_normal_block(row_offset + (uint64_t)i, (uint32_t)t, blk, seed_lo, seed_hi, nrm + 4 * blk);
            if (normals) memcpy(normals + it * POS_NORMALS, nrm, sizeof nrm);
            /* img_step under the recorded action: img1 on [stoch, action], the GRU as ps_act's, img2, img3 */
            memcpy(in1, st, PS_STOCH * sizeof(float));
            for (int j = 0; j < 2; ++j) st[PIS_FEAT + j] = in1[30 + j] = pis_clamp(actions[2 * it + j]);
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
            ps_dense(feat, 200, hd->img2_w, 200, 0, hd->img2_b, 200, x);
            for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
            ps_dense(x, 200, hd->img3_w, 60, 0, hd->img3_b, 60, out);                        /* mean | raw std */
            for (int j = 0; j < PS_STOCH; ++j) {
                qm[j] = out[j];
                qs[j] = pss_softplus(out[PS_STOCH + j]) + 0.1f;
            }
            if (prior_mean) memcpy(prior_mean + it * PS_STOCH, qm, sizeof qm);
            if (prior_std) memcpy(prior_std + it * PS_STOCH, qs, sizeof qs);
            const float *mean = qm, *sd = qs;
            if (t < context) {
                /* obs_step on [deter', embed], as ps_act's */
                for (int k = 0; k < PS_BEAMS; ++k) feat[PS_DETER + k] = ps_preprocess(scan[it * PS_BEAMS + k]);
                ps_dense(feat, PS_DETER + PS_BEAMS, w->obs1_w, 200, 0, w->obs1_b, 200, x);
                for (int j = 0; j < 200; ++j) x[j] = ps_elu(x[j]);
                ps_dense(x, 200, w->obs2_w, 60, 0, w->obs2_b, 60, out);
                float s = 0.0f;
                for (int j = 0; j < PS_STOCH; ++j) {
                    pm[j] = out[j];
                    ps[j] = pss_softplus(out[PS_STOCH + j]) + 0.1f;
                    s = s + pos_kl_term(pm[j], ps[j], qm[j], qs[j]);
                }
                if (post_mean) memcpy(post_mean + it * PS_STOCH, pm, sizeof pm);
                if (post_std) memcpy(post_std + it * PS_STOCH, ps, sizeof ps);
                if (kl) kl[it] = s;
                mean = pm;
                sd = ps;
            }
            for (int j = 0; j < PS_STOCH; ++j) st[j] = mode == 1 ? fmaf(sd[j], nrm[j], mean[j]) : mean[j];
            memcpy(st + PS_STOCH, feat, PS_DETER * sizeof(float));
            if (features) memcpy(features + it * PIS_FEAT, st, PIS_FEAT * sizeof(float));
            if (reward) reward[it] = pis_reward(hd, st);
        }
        if (state_out) memcpy(state_out + (size_t)i * PS_STATE, st, sizeof st);
    }
}

/* kl [n] of n pairs of 30-dimensional diagonal normals, as pos_observe sums it */
void pos_kl(int n, const float *pm, const float *ps, const float *qm, const float *qs, float *kl) {
    for (int i = 0; i < n; ++i) {
        float s = 0.0f;
        for (int j = 0; j < PS_STOCH; ++j) s = s + pos_kl_term(pm[i * PS_STOCH + j], ps[i * PS_STOCH + j], qm[i * PS_STOCH + j], qs[i * PS_STOCH + j]);
        kl[i] = s;
    }
}

/* 4 n_blocks normals of step t of a row: blocks first_block .. */
void pos_normals(uint64_t row_id, uint32_t t, uint32_t first_block, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, float *out) {
    for (int b = 0; b < n_blocks; ++b) pos_normal_block(row_id, t, first_block + (uint32_t)b, seed_lo, seed_hi, out + 4 * b);
}
