/* The binary32 specification of the actor's fit (rc_policy_actor_fit_step, rc_policy_actor_forward), restated
 * for the CPU under the conventions of policy_fit_spec.c, which it includes unchanged - and through it the other specs - for ps_dense,
 * ps_elu, ps_tanh, ps_sigmoid, pss_softplus, pfs_tree, pfs_elu_grad, pfs_back, pfs_wgrad and the types of the optimizer and its
 * hyper-parameters.  It restates racing_dreamer_amd/csrc/racecar_fit.hip at four hidden layers and includes nothing of it.  The
 * network is the reference's plain ActionDecoder(2, 4, 400, 'tanh_normal'), 230 -> 400 -> 400 -> 400 -> 400 -> 4, ELU, init_std 5,
 * min_std 1e-4, mean_scale 5 (dreamer/models.py:535-560); the optimizer is actor_opt's (dreamer/dream.py:87-88: lr 8e-5, clip 1.0),
 * dreamer/tools.py:421-455 as in policy_fit_spec.c.  The closed-loop gradient through the dream is not part of it: the gradient with
 * respect to the actions comes from the caller (grad) or from target actions (target).
 *
 * One step on N rows (features [N][230], eps [N][2] or NULL, weight [N] or NULL, exactly one of target [N][2] and grad [N][2]):
 *   forward    a_{l+1} = elu(a_l W_l + b_l), l = 0 .. 3, and o[0..3] = a4 Wout + bout: bias first, then the k-ascending fmaf chain.
 *   action     th_j = tanh(o_j / 5); mu_j = 5 th_j; raw_j = o_{2+j} + raw_init_std; sd_j = softplus(raw_j) + 1e-4;
 *              u_j = fmaf(sd_j, eps_j, mu_j) - with eps NULL u_j = mu_j, which is what the agent computes in mode mean -; act_j = tanh(u_j).
 *   delta      target: d_j = act_j - target_j; ga_j = d_j, with a weight ga_j = w ga_j, then ga_j = ga_j inv_n (inv_n = 1.0f / (float)N);
 *                      the row's loss term l = 0.5 fmaf(d_1, d_1, d_0 d_0), with a weight l = w l; stored negated (the sum below is
 *                      negated again, as for the likelihoods of policy_fit_spec.c).
 *              grad:   ga_j = grad_j, with a weight ga_j = w ga_j; no inv_n; the loss term +0.
 *              du_j = ga_j (1 - act_j act_j);  delta o_j = du_j (1 - th_j th_j);  delta o_{2+j} = (du_j eps_j) sigmoid(raw_j), +0 with
 *              eps NULL: every written operator one rounding, left to right.
 *   backward   delta4_j = (fmaf chain from +0 over c = 0, 1, 2, 3 of delta o_c Wout[j][c]) elu'(a4_j); delta3, delta2, delta1 through
 *              W3^T, W2^T, W1^T as pfs_back; grad_features = delta1 W0^T, the same chain from zero over the 400 units above.
 *   gradients  G_l = [a_{l-1} | 1]^T delta_l, G_out [401][4]: the ten arrays one behind the other, [231][400] | 3 x [401][400] |
 *              [401][4] = 575 204 floats, each summed over the rows in pfs_wgrad's four chains.
 *   sums, skip, clip, Adam: policy_fit_spec.c's, over 575 204 elements; loss = (float)(-(tree of the stored terms / (double)N)). */
#include "policy_fit_spec.c"

#define PAFS_GL ((PFS_UNITS + 1) * PFS_UNITS)
#define PAFS_GO (PFS_G1 + 3 * PAFS_GL)              /* the output layer follows the four hidden layers */
#define PAFS_NOUT 4
#define PAFS_NG (PAFS_GO + (PFS_UNITS + 1) * PAFS_NOUT)      /* 575 204 */
#define PAFS_RAW_INIT_STD 0x1.3f913cp+2f            /* log(exp(5) - 1) rounded to binary32: policy_sample_spec.c's */

typedef struct pafs_actor {
    float *h_w[4], *h_b[4], *out_w, *out_b;         /* the checkpoint's h0_w .. hout_b, row-major, updated in place */
} pafs_actor;

int pafs_grad_size(void) { return PAFS_NG; }

/* the four hidden layers on one row: a [4][400]; o [4] */
static void pafs_hidden(const pafs_actor *ac, const float *feat, float *a, float *o) {
    ps_dense(feat, PFS_FEAT, ac->h_w[0], 400, 0, ac->h_b[0], 400, a);
    for (int j = 0; j < 400; ++j) a[j] = ps_elu(a[j]);
    for (int l = 1; l < 4; ++l) {
        float *x = a + (size_t)l * PFS_UNITS;
        ps_dense(x - PFS_UNITS, 400, ac->h_w[l], 400, 0, ac->h_b[l], 400, x);
        for (int j = 0; j < 400; ++j) x[j] = ps_elu(x[j]);
    }
    ps_dense(a + 3 * PFS_UNITS, 400, ac->out_w, PAFS_NOUT, 0, ac->out_b, PAFS_NOUT, o);
}

/* the tanh-normal action of one output pair; th, raw for the delta */
static float pafs_action(float o_mean, float o_std, const float *eps, float *mu, float *sd, float *th, float *raw) {
    *th = ps_tanh(o_mean / 5.0f);
    *mu = 5.0f * *th;
    *raw = o_std + PAFS_RAW_INIT_STD;
    *sd = pss_softplus(*raw) + 1e-4f;
    return ps_tanh(eps ? fmaf(*sd, *eps, *mu) : *mu);
}

/* The forward pass alone: action, mean, std [n][2], any may be NULL. */
void pafs_forward(const pafs_actor *ac, int n, const float *feat, const float *eps, float *action, float *mean, float *std) {
    float *a = (float *)malloc((size_t)4 * PFS_UNITS * sizeof(float));
    for (int i = 0; i < n; ++i) {
        float o[PAFS_NOUT];
        pafs_hidden(ac, feat + (size_t)i * PFS_FEAT, a, o);
        for (int j = 0; j < 2; ++j) {
            float mu, sd, th, raw;
            const float act = pafs_action(o[j], o[2 + j], eps ? eps + 2 * (size_t)i + j : NULL, &mu, &sd, &th, &raw);
            if (action) action[2 * (size_t)i + j] = act;
            if (mean) mean[2 * (size_t)i + j] = mu;
            if (std) std[2 * (size_t)i + j] = sd;
        }
    }
    free(a);
}

/* The forward and backward pass: grad [PAFS_NG] (before the clip), lterm [n], gfeat [n][230] or NULL, out [n][4] or NULL (the
 * output layer's o, for the tests' count of saturated rows). */
void pafs_gradient(const pafs_actor *ac, int n, const float *feat, const float *eps, const float *weight, const float *target,
                   const float *gact, float *grad, float *lterm, float *gfeat, float *out) {
    const size_t plane = (size_t)n * PFS_UNITS;
    float *act = (float *)malloc((8 * plane + (size_t)n * PAFS_NOUT) * sizeof(float));
    float *chains = (float *)malloc((size_t)4 * (PFS_UNITS + 1) * PFS_UNITS * sizeof(float));
    float *arow = (float *)malloc((size_t)4 * PFS_UNITS * sizeof(float));
    float *a[4], *d[4], *dout = act + 8 * plane;
    for (int l = 0; l < 4; ++l) {
        a[l] = act + (size_t)l * plane;
        d[l] = act + (size_t)(4 + l) * plane;
    }
    const float inv_n = 1.0f / (float)n;
    for (int i = 0; i < n; ++i) {
        float o[PAFS_NOUT], tmp[PFS_UNITS], diff[2] = {0.0f, 0.0f};
        float *dq = dout + (size_t)i * PAFS_NOUT;
        pafs_hidden(ac, feat + (size_t)i * PFS_FEAT, arow, o);
        for (int l = 0; l < 4; ++l) memcpy(a[l] + (size_t)i * PFS_UNITS, arow + (size_t)l * PFS_UNITS, PFS_UNITS * sizeof(float));
        if (out) memcpy(out + (size_t)i * PAFS_NOUT, o, sizeof o);
        for (int j = 0; j < 2; ++j) {
            float mu, sd, th, raw, ga;
            const float *e = eps ? eps + 2 * (size_t)i + j : NULL;
            const float av = pafs_action(o[j], o[2 + j], e, &mu, &sd, &th, &raw);
            if (gact) {
                ga = gact[2 * (size_t)i + j];
                if (weight) ga = weight[i] * ga;
            } else {
                diff[j] = av - target[2 * (size_t)i + j];
                ga = diff[j];
                if (weight) ga = weight[i] * ga;
                ga = ga * inv_n;
            }
            const float du = ga * (1.0f - av * av);
            dq[j] = du * (1.0f - th * th);
            dq[2 + j] = e ? (du * *e) * ps_sigmoid(raw) : 0.0f;
        }
        float l = 0.0f;
        if (!gact) {
            l = 0.5f * fmaf(diff[1], diff[1], diff[0] * diff[0]);
            if (weight) l = weight[i] * l;
            l = -l;
        }
        lterm[i] = l;
        float *g4 = d[3] + (size_t)i * PFS_UNITS;
        for (int j = 0; j < 400; ++j) {
            const float *wr = ac->out_w + (size_t)j * PAFS_NOUT;
            float s = fmaf(dq[0], wr[0], 0.0f);
            s = fmaf(dq[1], wr[1], s);
            s = fmaf(dq[2], wr[2], s);
            s = fmaf(dq[3], wr[3], s);
            g4[j] = s * pfs_elu_grad(arow[3 * PFS_UNITS + j]);
        }
        for (int l2 = 2; l2 >= 0; --l2) {                                /* delta_{l2+1} from delta_{l2+2} through W_{l2+1}^T */
            float *g = d[l2] + (size_t)i * PFS_UNITS;
            pfs_back(d[l2 + 1] + (size_t)i * PFS_UNITS, ac->h_w[l2 + 1], 400, tmp);
            for (int j = 0; j < 400; ++j) g[j] = tmp[j] * pfs_elu_grad(arow[(size_t)l2 * PFS_UNITS + j]);
        }
        if (gfeat) pfs_back(d[0] + (size_t)i * PFS_UNITS, ac->h_w[0], PFS_FEAT, gfeat + (size_t)i * PFS_FEAT);
    }
    pfs_wgrad(n, feat, PFS_FEAT, PFS_FEAT, d[0], PFS_UNITS, PFS_UNITS, chains, grad);
    for (int l = 1; l < 4; ++l) pfs_wgrad(n, a[l - 1], PFS_UNITS, PFS_UNITS, d[l], PFS_UNITS, PFS_UNITS, chains, grad + PFS_G1 + (size_t)(l - 1) * PAFS_GL);
    pfs_wgrad(n, a[3], PFS_UNITS, PFS_UNITS, dout, PAFS_NOUT, PAFS_NOUT, chains, grad + PAFS_GO);
    free(arow);
    free(chains);
    free(act);
}

/* the weight behind gradient element e */
static float *pafs_weight(const pafs_actor *ac, int e) {
    if (e >= PAFS_GO) return e - PAFS_GO < PFS_UNITS * PAFS_NOUT ? ac->out_w + (e - PAFS_GO) : ac->out_b + (e - PAFS_GO - PFS_UNITS * PAFS_NOUT);
    const int l = e < PFS_G1 ? 0 : 1 + (e - PFS_G1) / PAFS_GL;
    const int i = e - (l == 0 ? 0 : PFS_G1 + (l - 1) * PAFS_GL), K = l == 0 ? PFS_FEAT : PFS_UNITS;
    return i < K * PFS_UNITS ? ac->h_w[l] + i : ac->h_b[l] + (i - K * PFS_UNITS);
}

/* One step: pfs_step over the actor.  opt->m, opt->v [PAFS_NG].  grad_out [PAFS_NG] or NULL: the gradient before the clip; gfeat
 * [n][230] or NULL; out [n][4] or NULL.  status [4] = loss, grad_norm, skipped, step. */
void pafs_step(const pafs_actor *ac, pfs_opt *opt, int n, const float *feat, const float *eps, const float *weight, const float *target,
               const float *gact, const pfs_hyper *hp, float *grad_out, float *gfeat, float *out, float *status) {
    float *grad = (float *)malloc((size_t)PAFS_NG * sizeof(float)), *lterm = (float *)malloc((size_t)n * sizeof(float));
    pafs_gradient(ac, n, feat, eps, weight, target, gact, grad, lterm, gfeat, out);
    if (grad_out) memcpy(grad_out, grad, (size_t)PAFS_NG * sizeof(float));
    const float norm = (float)sqrt(pfs_tree(grad, PAFS_NG, 1));
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
        for (int e = 0; e < PAFS_NG; ++e) {
            float *w = pafs_weight(ac, e);
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
