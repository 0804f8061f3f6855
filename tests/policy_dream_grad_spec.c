/* The binary32 specification of the dream's backward pass (rc_policy_dream_grad), restated for the CPU under
 * the conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is meant; built
 * with -ffp-contract=off -fno-fast-math by tests/policy_dream_grad_spec.py).  It includes policy_dream_spec.c - and through it the
 * specs below it - unchanged for the scalar functions, the dense chains, the normals and the tag-7 keying; the forward is
 * pds_dream's loop with every activation the backward needs kept per step, the backward restates
 * racing_dreamer_amd/csrc/racecar_dream_grad.hip; it includes neither.  This file is the authority for the order of operations
 * inside each elementwise expression. */
#include "policy_dream_spec.c"
#include <stdlib.h>

#define PDG_MAX_H 64

static float pdg_elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }        /* from the stored activation */

/* out[i] = 0, then for k ascending out[i] = fmaf(d[k], w[i][col0 + k], out[i]): the transposed product, one chain per input unit */
static void pdg_dense_t(const float *d, int k_n, const float *w, int ld, int col0, int n, float *out) {
    for (int i = 0; i < n; ++i) {
        float acc = 0.0f;
        const float *row = w + (size_t)i * ld + col0;
        for (int k = 0; k < k_n; ++k) acc = fmaf(d[k], row[k], acc);
        out[i] = acc;
    }
}

typedef struct pdg_step {
    float x1[PS_DETER], z[PS_DETER], r[PS_DETER], c[PS_DETER], hh[PS_DETER], h[PS_DETER], x2[PS_DETER], raw[PS_STOCH], nrm[PDS_NORMALS];
    float a1[PS_UNITS], a2[PS_UNITS], wgt;
} pdg_step;

/* H steps of K candidates of starts [0, n), forward as pds_dream and backward from the return: state [n][232], ids [n], actions_in
 * [n][K][H][2] raw.  Outputs, each optional: ret [n][K], reward [n][K][H], grad_actions [n][K][H][2] = d ret / d raw action,
 * grad_state [n][K][230] = d ret / d (stoch | deter) of the start. */
void pdg_dream_grad(const ps_weights *w, const pis_heads *hd, int mode, uint32_t seed_lo, uint32_t seed_hi, int n, int K, int k0, int k1, int H,
                    float discount, const float *state, const uint64_t *ids, const float *actions_in, float *ret, float *reward,
                    float *grad_actions, float *grad_state) {
    pdg_step *S = (pdg_step *)malloc(sizeof(pdg_step) * PDG_MAX_H);
    for (int i = 0; i < n; ++i) {
        for (int k = k0; k < k1; ++k) {
            const size_t q = (size_t)i * K + k;
            float st[PIS_FEAT];
            memcpy(st, state + (size_t)i * PS_STATE, sizeof st);
            float acc = 0.0f, wgt = 1.0f;
            for (int t = 0; t < H; ++t) {
                const size_t it = q * H + t;
                pdg_step *s = S + t;
                float in1[32], mx[600], mh[600], out[60], deter[PS_DETER], r1;
                memset(s->nrm, 0, sizeof s->nrm);
                if (mode == 1)
                    for (uint32_t blk = 0; blk < 8; ++blk) pds_normal_block(ids[i], (uint32_t)k, (uint32_t)t, blk, seed_lo, seed_hi, s->nrm + 4 * blk);
                memcpy(in1, st, PS_STOCH * sizeof(float));
                for (int j = 0; j < 2; ++j) in1[30 + j] = pis_clamp(actions_in[2 * it + j]);
                ps_dense(in1, 32, w->img1_w, 200, 0, w->img1_b, 200, s->x1);
                for (int j = 0; j < 200; ++j) s->x1[j] = ps_elu(s->x1[j]);
                memcpy(s->h, st + PS_STOCH, sizeof s->h);
                ps_dense(s->x1, 200, w->gru_kernel, 600, 0, w->gru_bias, 600, mx);
                ps_dense(s->h, 200, w->gru_recurrent, 600, 0, w->gru_bias + 600, 600, mh);
                for (int j = 0; j < 200; ++j) {
                    s->z[j] = ps_sigmoid(mx[j] + mh[j]);
                    s->r[j] = ps_sigmoid(mx[200 + j] + mh[200 + j]);
                    s->hh[j] = mh[400 + j];
                    s->c[j] = ps_tanh(mx[400 + j] + s->r[j] * s->hh[j]);
                    deter[j] = s->z[j] * s->h[j] + (1.0f - s->z[j]) * s->c[j];
                }
                ps_dense(deter, 200, hd->img2_w, 200, 0, hd->img2_b, 200, s->x2);
                for (int j = 0; j < 200; ++j) s->x2[j] = ps_elu(s->x2[j]);
                ps_dense(s->x2, 200, hd->img3_w, 60, 0, hd->img3_b, mode == 1 ? 60 : PS_STOCH, out);
                for (int j = 0; j < PS_STOCH; ++j) {
                    s->raw[j] = mode == 1 ? out[PS_STOCH + j] : 0.0f;
                    st[j] = mode == 1 ? fmaf(pss_softplus(out[PS_STOCH + j]) + 0.1f, s->nrm[j], out[j]) : out[j];
                }
                memcpy(st + PS_STOCH, deter, sizeof deter);
                /* the reward head, pis_reward's chains with both activations kept */
                ps_dense(st, PIS_FEAT, hd->rh0_w, 400, 0, hd->rh0_b, 400, s->a1);
                for (int j = 0; j < 400; ++j) s->a1[j] = ps_elu(s->a1[j]);
                ps_dense(s->a1, 400, hd->rh1_w, 400, 0, hd->rh1_b, 400, s->a2);
                for (int j = 0; j < 400; ++j) s->a2[j] = ps_elu(s->a2[j]);
                ps_dense(s->a2, 400, hd->rout_w, 1, 0, hd->rout_b, 1, &r1);
                if (reward) reward[it] = r1;
                acc = fmaf(wgt, r1, acc);
                s->wgt = wgt;
                wgt = wgt * discount;
            }
            if (ret) ret[q] = acc;
            /* backward: g = the cotangent on the feature after step t (stoch | deter), zero beyond H - 1 */
            float carry[PIS_FEAT];
            memset(carry, 0, sizeof carry);
            for (int t = H - 1; t >= 0; --t) {
                const size_t it = q * H + t;
                const pdg_step *s = S + t;
                float d2[PS_UNITS], d1[PS_UNITS], g[PIS_FEAT], in3[60], dx2[PS_DETER], dd[PS_DETER], gates[800], dx1[PS_DETER], din[32], rec[PS_DETER];
                /* 1. head */
                for (int j = 0; j < 400; ++j) d2[j] = fmaf(s->wgt, hd->rout_w[j], 0.0f) * pdg_elu_grad(s->a2[j]);
                pdg_dense_t(d2, 400, hd->rh1_w, 400, 0, 400, d1);
                for (int j = 0; j < 400; ++j) d1[j] = d1[j] * pdg_elu_grad(s->a1[j]);
                pdg_dense_t(d1, 400, hd->rh0_w, 400, 0, PIS_FEAT, g);
                /* 2. accumulate: head first */
                for (int j = 0; j < PIS_FEAT; ++j) g[j] = g[j] + carry[j];
                /* 3. stoch': mean | raw */
                for (int j = 0; j < PS_STOCH; ++j) {
                    in3[j] = g[j];
                    in3[PS_STOCH + j] = mode == 1 ? (g[j] * s->nrm[j]) * ps_sigmoid(s->raw[j]) : 0.0f;
                }
                /* 4. img3 (mode mean: the 30 mean columns only) */
                pdg_dense_t(in3, mode == 1 ? 60 : PS_STOCH, hd->img3_w, 60, 0, 200, dx2);
                for (int j = 0; j < 200; ++j) dx2[j] = dx2[j] * pdg_elu_grad(s->x2[j]);
                /* 5. img2 */
                pdg_dense_t(dx2, 200, hd->img2_w, 200, 0, 200, dd);
                for (int j = 0; j < 200; ++j) dd[j] = dd[j] + g[PS_STOCH + j];
                /* 6. GRU: gates = dz | dr | dc | dhh */
                for (int j = 0; j < 200; ++j) {
                    const float z = s->z[j], r = s->r[j], c = s->c[j];
                    const float dz = ((dd[j] * (s->h[j] - c)) * z) * (1.0f - z);
                    const float dc = (dd[j] * (1.0f - z)) * (1.0f - c * c);
                    gates[j] = dz;
                    gates[200 + j] = ((dc * s->hh[j]) * r) * (1.0f - r);
                    gates[400 + j] = dc;
                    gates[600 + j] = dc * r;
                }
                pdg_dense_t(gates, 600, w->gru_kernel, 600, 0, 200, dx1);
                for (int j = 0; j < 200; ++j) dx1[j] = dx1[j] * pdg_elu_grad(s->x1[j]);
                memcpy(gates + 400, gates + 600, 200 * sizeof(float));                       /* dz | dr | dhh */
                pdg_dense_t(gates, 600, w->gru_recurrent, 600, 0, 200, rec);
                for (int j = 0; j < 200; ++j) carry[PS_STOCH + j] = fmaf(dd[j], s->z[j], rec[j]);
                /* 7. img1 */
                pdg_dense_t(dx1, 200, w->img1_w, 200, 0, 32, din);
                memcpy(carry, din, PS_STOCH * sizeof(float));
                if (grad_actions)
                    for (int j = 0; j < 2; ++j) {
                        const float a = actions_in[2 * it + j];
                        grad_actions[2 * it + j] = (a >= -1.0f && a <= 1.0f) ? din[30 + j] : 0.0f;
                    }
            }
            if (grad_state) memcpy(grad_state + q * PIS_FEAT, carry, sizeof carry);
        }
    }
    free(S);
}
