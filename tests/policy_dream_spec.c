/* The binary32 specification of planning in the latent (rc_policy_dream_ahead), restated for the CPU under the
 * conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is meant; built
 * with -ffp-contract=off -fno-fast-math by tests/policy_dream_spec.py).  It includes policy_imagine_spec.c - and through it
 * policy_sample_spec.c and policy_spec.c - unchanged for the scalar functions, the dense chains, Philox, the normals and the reward
 * head, and restates the loop of racing_dreamer_amd/csrc/racecar_dream.hip, its return and the tag-7 keying of
 * racecar_policy_math.h; it includes neither. */
#include "policy_imagine_spec.c"

#define PDS_NORMALS 32           /* per row and step: blocks 0-7 (30 used) */

/* id = the start's 64-bit id, cand = the candidate, t = the step */
void pds_normal_block(uint64_t id, uint32_t cand, uint32_t t, uint32_t block, uint32_t seed_lo, uint32_t seed_hi, float n[4]) {
    uint32_t r[4];
    pss_philox((uint32_t)id, (uint32_t)(id >> 32), cand, block | (t << 8) | (7u << 24), seed_lo, seed_hi, r);
    pss_normal_pair(r[0], r[1], &n[0], &n[1]);
    pss_normal_pair(r[2], r[3], &n[2], &n[3]);
}

/* H steps of K candidates of starts [0, n) in mode 0 (mean) or 1 (sample): state [n][232] (stoch | deter | not read), ids [n] the
 * starts' ids, actions_in [n][K][H][2] raw.  Candidates [k0, k1) are computed (the draws do not know K; their rows are written at
 * their place among the K).  Outputs, each optional: ret [n][K], reward [n][K][H] (both need the head), final_feature [n][K][230],
 * normals [n][K][H][PDS_NORMALS], means / stds [n][K][H][30] (the prior's mean and std of each step). */
void pds_dream(const ps_weights *w, const pis_heads *hd, int mode, uint32_t seed_lo, uint32_t seed_hi, int n, int K, int k0, int k1, int H,
               float discount, const float *state, const uint64_t *ids, const float *actions_in, float *ret, float *reward,
               float *final_feature, float *normals, float *means, float *stds) {
    for (int i = 0; i < n; ++i) {
        for (int k = k0; k < k1; ++k) {
            const size_t q = (size_t)i * K + k;
            float st[PIS_FEAT];
            memcpy(st, state + (size_t)i * PS_STATE, sizeof st);
            float acc = 0.0f, wgt = 1.0f;
            for (int t = 0; t < H; ++t) {
                const size_t it = q * H + t;
                float nrm[PDS_NORMALS], in1[32], x[PS_DETER], mx[600], mh[600], out[60], deter[PS_DETER];
                memset(nrm, 0, sizeof nrm);
                if (mode == 1)
                    for (uint32_t blk = 0; blk < 8; ++blk) pds_normal_block(ids[i], (uint32_t)k, (uint32_t)t, blk, seed_lo, seed_hi, nrm + 4 * blk);
                if (normals) memcpy(normals + it * PDS_NORMALS, nrm, sizeof nrm);
                /* img_step under the candidate's action: img1 on [stoch, action], the GRU as ps_act's, img2, img3 */
                memcpy(in1, st, PS_STOCH * sizeof(float));
                for (int j = 0; j < 2; ++j) in1[30 + j] = pis_clamp(actions_in[2 * it + j]);
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
                ps_dense(x, 200, hd->img3_w, 60, 0, hd->img3_b, (mode == 1 || stds) ? 60 : PS_STOCH, out);        /* mean | raw std */
                for (int j = 0; j < PS_STOCH; ++j) {
                    const float sd = (mode == 1 || stds) ? pss_softplus(out[PS_STOCH + j]) + 0.1f : 0.0f;
                    if (means) means[it * PS_STOCH + j] = out[j];
                    if (stds) stds[it * PS_STOCH + j] = sd;
                    st[j] = mode == 1 ? fmaf(sd, nrm[j], out[j]) : out[j];
                }
                memcpy(st + PS_STOCH, deter, sizeof deter);
                if (ret || reward) {
                    const float r = pis_reward(hd, st);
                    if (reward) reward[it] = r;
                    acc = fmaf(wgt, r, acc);
                    wgt = wgt * discount;
                }
            }
            if (ret) ret[q] = acc;
            if (final_feature) memcpy(final_feature + q * PIS_FEAT, st, sizeof st);
        }
    }
}

/* ret [n] of n reward rows [n][H] under `discount`, as pds_dream accumulates it */
void pds_return(int n, int H, float discount, const float *reward, float *ret) {
    for (int i = 0; i < n; ++i) {
        float acc = 0.0f, wgt = 1.0f;
        for (int t = 0; t < H; ++t) {
            acc = fmaf(wgt, reward[(size_t)i * H + t], acc);
            wgt = wgt * discount;
        }
        ret[i] = acc;
    }
}

/* 4 n_blocks normals of step t of candidate cand of the start id: blocks first_block .. */
void pds_normals(uint64_t id, uint32_t cand, uint32_t t, uint32_t first_block, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, float *out) {
    for (int b = 0; b < n_blocks; ++b) pds_normal_block(id, cand, t, first_block + (uint32_t)b, seed_lo, seed_hi, out + 4 * b);
}
