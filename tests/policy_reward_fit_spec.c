/* The binary32 specification of the reward head's fit (rc_policy_fit_step with RC_POLICY_FIT_REWARD), restated
 * for the CPU under the conventions of policy_fit_spec.c, which it includes unchanged - and through it the other specs - for
 * ps_dense, ps_elu, pfs_tree, pfs_elu_grad, pfs_back, pfs_wgrad and the types of the optimizer and its hyper-parameters.  It restates
 * racing_dreamer_amd/csrc/racecar_fit.hip at two hidden layers and includes nothing of it.  The head is the reference's
 * DenseDecoder((), 2, 400) (dreamer/models.py:167), 230 -> 400 -> 400 -> 1, under Normal(o, 1) against the recorded reward
 * (models.py:97-100); the optimizer is dreamer/tools.py:421-455 as in policy_fit_spec.c.
 *
 * What two layers change against policy_fit_spec.c's value head, and nothing else does:
 *   forward    a1 = elu(a0 W0 + b0), a2 = elu(a1 W1 + b1), o = a2 Wout + bout.
 *   loss term  the value head's: e = o - t, lp = fmaf(-0.5, e e, -log(2 pi) / 2); with a weight e = w e, lp = w lp; delta_o = e inv_n.
 *   backward   delta2 = fmaf(delta_o, Wout[j], 0) elu'(a2[j]); delta1 = (delta2 W1^T) elu'(a1).
 *   gradients  G_0 [231][400] = [a0 | 1]^T delta1, G_1 [401][400] = [a1 | 1]^T delta2, G_out [401][1] = [a2 | 1]^T delta_o: the six
 *              arrays one behind the other, 253 201 floats, each summed over the rows in pfs_wgrad's four chains.
 *   sums, skip, clip, Adam: policy_fit_spec.c's, over 253 201 elements (the loop of pfs_step, restated here because that one is
 *              written over the value head's 413 601 and its element-to-weight map). */
#include "policy_fit_spec.c"

#define PRFS_GO PFS_G2                              /* the output layer follows the two hidden layers */
#define PRFS_NG (PRFS_GO + PFS_UNITS + 1)           /* 253 201 */

typedef struct prfs_head {
    float *h_w[2], *h_b[2], *out_w, *out_b;         /* the checkpoint's reward_* arrays, row-major, updated in place */
} prfs_head;

int prfs_grad_size(void) { return PRFS_NG; }

/* The forward and backward pass: grad [PRFS_NG] (before the clip), lterm [n]. */
void prfs_gradient(const prfs_head *hd, int n, const float *feat, const float *target, const float *weight, float *grad, float *lterm) {
    const size_t plane = (size_t)n * PFS_UNITS;
    float *buf = (float *)malloc((4 * plane + (size_t)n) * sizeof(float));
    float *chains = (float *)malloc((size_t)4 * (PFS_UNITS + 1) * PFS_UNITS * sizeof(float));
    float *a1 = buf, *a2 = buf + plane, *d1 = buf + 2 * plane, *d2 = buf + 3 * plane, *dout = buf + 4 * plane;
    const float inv_n = 1.0f / (float)n;
    for (int i = 0; i < n; ++i) {
        float *x1 = a1 + (size_t)i * PFS_UNITS, *x2 = a2 + (size_t)i * PFS_UNITS, o, tmp[PFS_UNITS];
        ps_dense(feat + (size_t)i * PFS_FEAT, PFS_FEAT, hd->h_w[0], 400, 0, hd->h_b[0], 400, x1);
        for (int j = 0; j < 400; ++j) x1[j] = ps_elu(x1[j]);
        ps_dense(x1, 400, hd->h_w[1], 400, 0, hd->h_b[1], 400, x2);
        for (int j = 0; j < 400; ++j) x2[j] = ps_elu(x2[j]);
        ps_dense(x2, 400, hd->out_w, 1, 0, hd->out_b, 1, &o);
        float e = o - target[i];
        float lp = fmaf(-0.5f, e * e, -0.9189385332f);
        if (weight) {
            e = weight[i] * e;
            lp = weight[i] * lp;
        }
        const float delta = e * inv_n;
        dout[i] = delta;
        lterm[i] = lp;
        float *g2 = d2 + (size_t)i * PFS_UNITS, *g1 = d1 + (size_t)i * PFS_UNITS;
        for (int j = 0; j < 400; ++j) g2[j] = fmaf(delta, hd->out_w[j], 0.0f) * pfs_elu_grad(x2[j]);
        pfs_back(g2, hd->h_w[1], 400, tmp);
        for (int j = 0; j < 400; ++j) g1[j] = tmp[j] * pfs_elu_grad(x1[j]);
    }
    pfs_wgrad(n, feat, PFS_FEAT, PFS_FEAT, d1, PFS_UNITS, PFS_UNITS, chains, grad);
    pfs_wgrad(n, a1, PFS_UNITS, PFS_UNITS, d2, PFS_UNITS, PFS_UNITS, chains, grad + PFS_G1);
    pfs_wgrad(n, a2, PFS_UNITS, PFS_UNITS, dout, 1, 1, chains, grad + PRFS_GO);
    free(chains);
    free(buf);
}

/* the weight behind gradient element e */
static float *prfs_weight(const prfs_head *hd, int e) {
    if (e >= PRFS_GO) return e - PRFS_GO < PFS_UNITS ? hd->out_w + (e - PRFS_GO) : hd->out_b;
    const int l = e < PFS_G1 ? 0 : 1;
    const int i = e - (l == 0 ? 0 : PFS_G1), K = l == 0 ? PFS_FEAT : PFS_UNITS;
    return i < K * PFS_UNITS ? hd->h_w[l] + i : hd->h_b[l] + (i - K * PFS_UNITS);
}

/* One step: pfs_step over the reward head.  opt->m, opt->v [PRFS_NG].  grad_out [PRFS_NG] or NULL: the gradient before the clip.
 * status [4] = loss, grad_norm, skipped, step. */
void prfs_step(const prfs_head *hd, pfs_opt *opt, int n, const float *feat, const float *target, const float *weight, const pfs_hyper *hp,
               float *grad_out, float *status) {
    float *grad = (float *)malloc((size_t)PRFS_NG * sizeof(float)), *lterm = (float *)malloc((size_t)n * sizeof(float));
    prfs_gradient(hd, n, feat, target, weight, grad, lterm);
    if (grad_out) memcpy(grad_out, grad, (size_t)PRFS_NG * sizeof(float));
    const float norm = (float)sqrt(pfs_tree(grad, PRFS_NG, 1));
    const float loss = (float)(-(pfs_tree(lterm, n, 0) / (double)n));
    const int finite = isfinite(norm) ? 1 : 0;
    if (finite) {
        opt->step += 1;
        opt->b1pow = opt->b1pow * (double)hp->beta1;
        opt->b2pow = opt->b2pow * (double)hp->beta2;
        const float c1 = (float)(1.0 - opt->b1pow), c2 = (float)(1.0 - opt->b2pow);
        const float lr_t = (hp->lr * sqrtf(c2)) / c1;
        const float scale = hp->clip > 0.0f ? hp->clip / (norm > hp->clip ? norm : hp->clip) : 1.0f;
        const float omb1 = 1.0f - hp->beta1, omb2 = 1.0f - hp->beta2;
        for (int e = 0; e < PRFS_NG; ++e) {
            float *w = prfs_weight(hd, e);
            const float g = grad[e] * scale;
            const float m = fmaf(hp->beta1, opt->m[e], omb1 * g);
            const float v = fmaf(hp->beta2, opt->v[e], omb2 * (g * g));
            const float den = sqrtf(v) + hp->epsilon;
            *w = fmaf(-lr_t, m / den, *w);
            opt->m[e] = m;
            opt->v[e] = v;
        }
    }
    status[0] = loss;
    status[1] = norm;
    status[2] = finite ? 0.0f : 1.0f;
    status[3] = (float)opt->step;
    free(lterm);
    free(grad);
}
