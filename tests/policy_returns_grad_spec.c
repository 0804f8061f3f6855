/* The binary32 specification of the actor loss's gradient through the dream (rc_policy_returns_grad), restated
 * for the CPU under the conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation
 * is meant; built with -O2 -ffp-contract=off -fno-fast-math by tests/policy_returns_grad_spec.py).  It includes policy_returns_spec.c -
 * and through it the specs below - unchanged for the scalar functions, the dense chains, the normals and both keyings; the forward is
 * prs_returns' loop with every activation the backward needs kept per step.  The backward of the prior step is
 * policy_dream_grad_spec.c's steps 2-7 (that file includes policy_dream_spec.c, which cannot be included beside policy_returns_spec.c:
 * both include policy_imagine_spec.c; its two helpers and its step are restated here, operator for operator), the heads' chains are
 * policy_fit_spec.c's delta chains.  It restates racing_dreamer_amd/csrc/racecar_returns_grad.hip and includes nothing of it.  This
 * file is the authority for the order of operations.
 *
 * The objective of a row: J = sum over t < H - 1 of (scale weight[t]) returns[t], weight held constant (the reference's
 * stop_gradient(cumprod), dreamer/models.py:121-127), returns differentiated through r, v and p.  The actor is NOT differentiated:
 * the reference feeds it stop_gradient(feat) (models.py:218-219), so the cotangent of a feature never enters the actor, and the
 * closed-loop backward pass is the open-loop one under the actions the actor produced.
 *
 *   coefficients   s_t = scale weight[t];  g_t = p_t lambda (the forward's rounding);  for t = 0 .. H - 2:
 *                    A_t = t == 0 ? s_0 : fmaf(A_{t-1}, g_{t-1}, s_t);   c_r[t] = A_t;
 *                    c_p[t] = A_t fmaf(lambda, R_{t+1}, v_{t+1} (1 - lambda))   (R_{H-1} = v_{H-1});
 *                    c_v[t+1] = (A_t p_t) (1 - lambda);
 *                  then c_v[H-1] = fmaf(A_{H-2}, g_{H-2}, (A_{H-2} p_{H-2}) (1 - lambda)).  No c_v[0], c_r[H-1], c_p[H-1]: those heads
 *                  are not run backward at those steps and add nothing.  The pcont logit's delta is c_p[t] (p_t (1 - p_t)); without
 *                  a pcont head p is the constant and has no gradient.
 *   backward       t = H - 1 .. 0: reward head (t < H - 1) delta2 = fmaf(c_r, rout_w[j], 0) elu'(a2), delta1 = (delta2 rh1^T) elu'(a1),
 *                  g = delta1 rh0^T; carry = g + carry.  Value head (t >= 1) from c_v[t] through three layers the same way; carry =
 *                  g + carry.  Pcont head (loaded, t < H - 1) from its logit delta; carry = g + carry.  Then stoch', img3, img2, the
 *                  GRU and img1 as item 23; grad_actions[t] = delta in[30:32], exactly +0 where a given raw action lies outside
 *                  [-1, 1] (bounds inclusive); no mask in closed loop. */
#include "policy_returns_spec.c"
#include <stdlib.h>

#define PRG_MAX_H 64

static float prg_elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }        /* from the stored activation */

/* out[i] = 0, then for k ascending out[i] = fmaf(d[k], w[i][k], out[i]): the transposed product, one chain per input unit */
static void prg_dense_t(const float *d, int k_n, const float *w, int ld, int n, float *out) {
    for (int i = 0; i < n; ++i) {
        float acc = 0.0f;
        const float *row = w + (size_t)i * ld;
        for (int k = 0; k < k_n; ++k) acc = fmaf(d[k], row[k], acc);
        out[i] = acc;
    }
}

typedef struct prg_step {
    float x1[PS_DETER], z[PS_DETER], r[PS_DETER], c[PS_DETER], hh[PS_DETER], h[PS_DETER], x2[PS_DETER], raw[PS_STOCH], nrm[PIS_NORMALS];
    float ra[2][PS_UNITS], va[3][PS_UNITS], pa[3][PS_UNITS];          /* the heads' activations on the feature after the step */
    float seen[PIS_FEAT];                                             /* the feature the actor read for a_t */
} prg_step;

/* DenseDecoder((), 3, 400) with the activations kept: prs_head3's chains */
static float prg_head3(const float *const hw[3], const float *const hb[3], const float *out_w, const float *out_b, const float *feat, float a[3][PS_UNITS]) {
    float r;
    ps_dense(feat, PIS_FEAT, hw[0], 400, 0, hb[0], 400, a[0]);
    for (int j = 0; j < 400; ++j) a[0][j] = ps_elu(a[0][j]);
    ps_dense(a[0], 400, hw[1], 400, 0, hb[1], 400, a[1]);
    for (int j = 0; j < 400; ++j) a[1][j] = ps_elu(a[1][j]);
    ps_dense(a[1], 400, hw[2], 400, 0, hb[2], 400, a[2]);
    for (int j = 0; j < 400; ++j) a[2][j] = ps_elu(a[2][j]);
    ps_dense(a[2], 400, out_w, 1, 0, out_b, 1, &r);
    return r;
}

/* a head's feature gradient from the cotangent `seed` of its one output: n_hidden layers above the first */
static void prg_head_back(float seed, const float *out_w, const float *const *hw, int n_layers, float (*a)[PS_UNITS], float *g) {
    float d[PS_UNITS], e[PS_UNITS];
    for (int j = 0; j < 400; ++j) d[j] = fmaf(seed, out_w[j], 0.0f) * prg_elu_grad(a[n_layers - 1][j]);
    for (int l = n_layers - 1; l >= 1; --l) {
        prg_dense_t(d, 400, hw[l], 400, 400, e);
        for (int j = 0; j < 400; ++j) d[j] = e[j] * prg_elu_grad(a[l - 1][j]);
    }
    prg_dense_t(d, 400, hw[0], 400, PIS_FEAT, g);
}

/* The coefficient series of one row: r is not read; v, p [H], ret [H - 1], weight [H - 1] the forward's -> c_r, c_p [H - 1], c_v [H]
 * (c_v[0] is not written) */
void prg_coefficients(int H, const float *v, const float *p, const float *ret, const float *weight, float lambda, float scale, float *c_r,
                      float *c_p, float *c_v) {
    const float oml = 1.0f - lambda;
    float A = 0.0f;
    for (int t = 0; t <= H - 2; ++t) {
        const float s = scale * weight[t];
        A = t == 0 ? s : fmaf(A, p[t - 1] * lambda, s);
        const float next = t + 1 < H - 1 ? ret[t + 1] : v[H - 1];
        c_r[t] = A;
        c_p[t] = A * fmaf(lambda, next, v[t + 1] * oml);
        c_v[t + 1] = (A * p[t]) * oml;
    }
    c_v[H - 1] = fmaf(A, p[H - 2] * lambda, (A * p[H - 2]) * oml);
}

/* H imagined steps for rows [0, n) and the gradient of J: prs_returns' arguments (the forward outputs come out as it gives them),
 * then scale and the outputs grad_actions [n][H][2], actor_features [n][H][230], eps [n][H][2], grad_state [n][230], each optional.
 * H >= 2; the reward head and the value head are needed. */
void prg_returns_grad(const ps_weights *w, const pis_heads *hd, const prs_critic *cr, int mode, uint32_t seed_lo, uint32_t seed_hi, int n, int H,
                      float lambda, float discount, float scale, const float *state, int keyed, const void *keys, const float *actions_in,
                      float *reward, float *value, float *pcont, float *ret, float *weight, float *actions, float *features, float *start,
                      int n_start, float *normals, float *grad_actions, float *actor_features, float *eps, float *grad_state) {
    prg_step *S = (prg_step *)malloc(sizeof(prg_step) * PRG_MAX_H);
    const float *const vhw[3] = {cr->vh_w[0], cr->vh_w[1], cr->vh_w[2]}, *const vhb[3] = {cr->vh_b[0], cr->vh_b[1], cr->vh_b[2]};
    const float *const phw[3] = {cr->ph_w[0], cr->ph_w[1], cr->ph_w[2]}, *const phb[3] = {cr->ph_b[0], cr->ph_b[1], cr->ph_b[2]};
    const float *const rhw[2] = {hd->rh0_w, hd->rh1_w};
    for (int i = 0; i < n; ++i) {
        float st[PIS_FEAT], rs[PRG_MAX_H], vs[PRG_MAX_H], ps[PRG_MAX_H], Rs[PRG_MAX_H], ws[PRG_MAX_H];
        memcpy(st, state + (size_t)i * PS_STATE, sizeof st);
        const uint32_t *key = keyed ? NULL : (const uint32_t *)keys + 4 * (size_t)i;
        const uint64_t id = keyed ? ((const uint64_t *)keys)[i] : 0;
        if (start) {
            start[i] = pis_reward(hd, st);
            start[(size_t)n_start + i] = prs_head3(cr->vh_w, cr->vh_b, cr->vout_w, cr->vout_b, st);
            if (cr->pout_w) start[2 * (size_t)n_start + i] = ps_sigmoid(prs_head3(cr->ph_w, cr->ph_b, cr->pout_w, cr->pout_b, st));
        }
        /* ---- forward: prs_returns' step, the activations kept */
        for (int t = 0; t < H; ++t) {
            const size_t it = (size_t)i * H + t;
            prg_step *s = S + t;
            float in1[32], mx[600], mh[600], a[PS_UNITS], b[PS_UNITS], out[60], deter[PS_DETER];
            memset(s->nrm, 0, sizeof s->nrm);
            if (mode == 1) {
                for (uint32_t blk = 0; blk < 9; ++blk) {
                    if (blk == 8 && actions_in) break;
                    if (keyed) prs_normal_block(id, (uint32_t)t, blk, seed_lo, seed_hi, s->nrm + 4 * blk);
                    else pis_normal_block(key, (uint32_t)t, blk, seed_lo, seed_hi, s->nrm + 4 * blk);
                }
            }
            if (normals) memcpy(normals + it * PIS_NORMALS, s->nrm, sizeof s->nrm);
            memcpy(s->seen, st, sizeof st);
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
                    act[j] = mode == 1 ? ps_tanh(fmaf(sd, s->nrm[32 + j], mu)) : ps_tanh(mu);
                }
            }
            if (actions) { actions[2 * it] = act[0]; actions[2 * it + 1] = act[1]; }
            memcpy(in1, st, PS_STOCH * sizeof(float));
            in1[30] = act[0];
            in1[31] = act[1];
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
            if (features) memcpy(features + it * PIS_FEAT, st, sizeof st);
            /* the three heads on the new feature, pis_reward's and prs_head3's chains with the activations kept */
            ps_dense(st, PIS_FEAT, hd->rh0_w, 400, 0, hd->rh0_b, 400, s->ra[0]);
            for (int j = 0; j < 400; ++j) s->ra[0][j] = ps_elu(s->ra[0][j]);
            ps_dense(s->ra[0], 400, hd->rh1_w, 400, 0, hd->rh1_b, 400, s->ra[1]);
            for (int j = 0; j < 400; ++j) s->ra[1][j] = ps_elu(s->ra[1][j]);
            ps_dense(s->ra[1], 400, hd->rout_w, 1, 0, hd->rout_b, 1, &rs[t]);
            vs[t] = prg_head3(vhw, vhb, cr->vout_w, cr->vout_b, st, s->va);
            ps[t] = cr->pout_w ? ps_sigmoid(prg_head3(phw, phb, cr->pout_w, cr->pout_b, st, s->pa)) : discount;
            if (reward) reward[it] = rs[t];
            if (value) value[it] = vs[t];
            if (pcont) pcont[it] = ps[t];
        }
        prs_lambda_return(H, rs, vs, ps, lambda, Rs, ws);
        if (ret) memcpy(ret + (size_t)i * (H - 1), Rs, (size_t)(H - 1) * sizeof(float));
        if (weight) memcpy(weight + (size_t)i * (H - 1), ws, (size_t)(H - 1) * sizeof(float));
        if (actor_features)
            for (int t = 0; t < H; ++t) memcpy(actor_features + ((size_t)i * H + t) * PIS_FEAT, S[t].seen, sizeof S[t].seen);
        if (eps)
            for (int t = 0; t < H; ++t) { eps[2 * ((size_t)i * H + t)] = S[t].nrm[32]; eps[2 * ((size_t)i * H + t) + 1] = S[t].nrm[33]; }
        if (!grad_actions && !grad_state) continue;
        /* ---- the adjoint of the recursion */
        float c_r[PRG_MAX_H], c_p[PRG_MAX_H], c_v[PRG_MAX_H];
        prg_coefficients(H, vs, ps, Rs, ws, lambda, scale, c_r, c_p, c_v);
        /* ---- backward: carry = the cotangent on the feature after step t (stoch | deter), zero beyond H - 1 */
        float carry[PIS_FEAT];
        memset(carry, 0, sizeof carry);
        for (int t = H - 1; t >= 0; --t) {
            const size_t it = (size_t)i * H + t;
            prg_step *s = S + t;
            float g[PIS_FEAT], in3[60], dx2[PS_DETER], dd[PS_DETER], gates[800], dx1[PS_DETER], din[32], rec[PS_DETER];
            /* 1. the heads, each added head first: reward, value, pcont */
            if (t < H - 1) {
                prg_head_back(c_r[t], hd->rout_w, rhw, 2, s->ra, g);
                for (int j = 0; j < PIS_FEAT; ++j) carry[j] = g[j] + carry[j];
            }
            if (t >= 1) {
                prg_head_back(c_v[t], cr->vout_w, vhw, 3, s->va, g);
                for (int j = 0; j < PIS_FEAT; ++j) carry[j] = g[j] + carry[j];
            }
            if (cr->pout_w && t < H - 1) {
                prg_head_back(c_p[t] * (ps[t] * (1.0f - ps[t])), cr->pout_w, phw, 3, s->pa, g);
                for (int j = 0; j < PIS_FEAT; ++j) carry[j] = g[j] + carry[j];
            }
            memcpy(g, carry, sizeof g);
            /* 3. stoch': mean | raw */
            for (int j = 0; j < PS_STOCH; ++j) {
                in3[j] = g[j];
                in3[PS_STOCH + j] = mode == 1 ? (g[j] * s->nrm[j]) * ps_sigmoid(s->raw[j]) : 0.0f;
            }
            /* 4. img3 (mode mean: the 30 mean columns only) */
            prg_dense_t(in3, mode == 1 ? 60 : PS_STOCH, hd->img3_w, 60, 200, dx2);
            for (int j = 0; j < 200; ++j) dx2[j] = dx2[j] * prg_elu_grad(s->x2[j]);
            /* 5. img2 */
            prg_dense_t(dx2, 200, hd->img2_w, 200, 200, dd);
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
            prg_dense_t(gates, 600, w->gru_kernel, 600, 200, dx1);
            for (int j = 0; j < 200; ++j) dx1[j] = dx1[j] * prg_elu_grad(s->x1[j]);
            memcpy(gates + 400, gates + 600, 200 * sizeof(float));                       /* dz | dr | dhh */
            prg_dense_t(gates, 600, w->gru_recurrent, 600, 200, rec);
            for (int j = 0; j < 200; ++j) carry[PS_STOCH + j] = fmaf(dd[j], s->z[j], rec[j]);
            /* 7. img1 */
            prg_dense_t(dx1, 200, w->img1_w, 200, 32, din);
            memcpy(carry, din, PS_STOCH * sizeof(float));
            if (grad_actions)
                for (int j = 0; j < 2; ++j) {
                    float ga = din[30 + j];
                    if (actions_in) {
                        const float a = actions_in[2 * it + j];
                        ga = (a >= -1.0f && a <= 1.0f) ? ga : 0.0f;
                    }
                    grad_actions[2 * it + j] = ga;
                }
        }
        if (grad_state) memcpy(grad_state + (size_t)i * PIS_FEAT, carry, sizeof carry);
    }
    free(S);
}
