/* The binary32 specification of the actor's fit (rc_policy_actor_fit_step, rc_policy_actor_forward): the fit
 * engine of policy_fit_spec.c, which it includes unchanged - and through it the other specs -, at four hidden layers and four
 * outputs under the actor's own output rule.  It restates racing_dreamer_amd/csrc/racecar_fit.hip at four hidden layers and includes
 * nothing of it.  The network is the reference's plain ActionDecoder(2, 4, 400, 'tanh_normal'), 230 -> 400 -> 400 -> 400 -> 400 -> 4,
 * ELU, init_std 5, min_std 1e-4, mean_scale 5 (dreamer/models.py:535-560); the optimizer is actor_opt's (dreamer/dream.py:87-88:
 * lr 8e-5, clip 1.0), dreamer/tools.py:421-455 as in policy_fit_spec.c.  The closed-loop gradient through the dream is not part of
 * it: the gradient with respect to the actions comes from the caller (grad) or from target actions (target).
 *
 * What the rule is, on N rows (eps [N][2] or NULL, weight [N] or NULL, exactly one of target [N][2] and grad [N][2]); forward,
 * backward (with grad_features), gradients, sums, skip, clip and Adam are the engine's at D = 4, W = 4, 575 204 elements:
 *   action     th_j = tanh(o_j / 5); mu_j = 5 th_j; raw_j = o_{2+j} + raw_init_std; sd_j = softplus(raw_j) + 1e-4;
 *              u_j = fmaf(sd_j, eps_j, mu_j) - with eps NULL u_j = mu_j, which is what the agent computes in mode mean -; act_j = tanh(u_j).
 *   delta      target: d_j = act_j - target_j; ga_j = d_j, with a weight ga_j = w ga_j, then ga_j = ga_j inv_n (inv_n = 1.0f / (float)N);
 *                      the row's loss term l = 0.5 fmaf(d_1, d_1, d_0 d_0), with a weight l = w l; stored negated (the engine's sum is
 *                      negated again, as for the likelihoods of policy_fit_spec.c).
 *              grad:   ga_j = grad_j, with a weight ga_j = w ga_j; no inv_n; the loss term +0.
 *              du_j = ga_j (1 - act_j act_j);  delta o_j = du_j (1 - th_j th_j);  delta o_{2+j} = (du_j eps_j) sigmoid(raw_j), +0 with
 *              eps NULL: every written operator one rounding, left to right. */
#include "policy_fit_spec.c"

#define PAFS_RAW_INIT_STD 0x1.3f913cp+2f            /* log(exp(5) - 1) rounded to binary32: policy_sample_spec.c's */

/* the tanh-normal action of one output pair; th, raw for the delta */
static float pafs_action(float o_mean, float o_std, const float *eps, float *mu, float *sd, float *th, float *raw) {
    *th = ps_tanh(o_mean / 5.0f);
    *mu = 5.0f * *th;
    *raw = o_std + PAFS_RAW_INIT_STD;
    *sd = pss_softplus(*raw) + 1e-4f;
    return ps_tanh(eps ? fmaf(*sd, *eps, *mu) : *mu);
}

/* The forward pass alone: action, mean, std [n][2], any may be NULL. */
void pafs_forward(const pfs_net *ac, int n, const float *feat, const float *eps, float *action, float *mean, float *std) {
    float *a = (float *)malloc((size_t)PFS_MAX_DEPTH * PFS_UNITS * sizeof(float)), *row[PFS_MAX_DEPTH];
    for (int l = 0; l < PFS_MAX_DEPTH; ++l) row[l] = a + (size_t)l * PFS_UNITS;
    for (int i = 0; i < n; ++i) {
        float o[PFS_MAX_OUT];
        pfs_forward_row(ac, feat + (size_t)i * PFS_FEAT, row, o);
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

/* the actor's rule: rw->grad given: grad mode, else target mode */
static float pafs_rule(const pfs_rows *rw, int i, float inv_n, const float *o, float *delta_o) {
    float diff[2] = {0.0f, 0.0f};
    for (int j = 0; j < 2; ++j) {
        float mu, sd, th, raw, ga;
        const float *e = rw->eps ? rw->eps + 2 * (size_t)i + j : NULL;
        const float av = pafs_action(o[j], o[2 + j], e, &mu, &sd, &th, &raw);
        if (rw->grad) {
            ga = rw->grad[2 * (size_t)i + j];
            if (rw->weight) ga = rw->weight[i] * ga;
        } else {
            diff[j] = av - rw->target[2 * (size_t)i + j];
            ga = diff[j];
            if (rw->weight) ga = rw->weight[i] * ga;
            ga = ga * inv_n;
        }
        const float du = ga * (1.0f - av * av);
        delta_o[j] = du * (1.0f - th * th);
        delta_o[2 + j] = e ? (du * *e) * ps_sigmoid(raw) : 0.0f;
    }
    float l = 0.0f;
    if (!rw->grad) {
        l = 0.5f * fmaf(diff[1], diff[1], diff[0] * diff[0]);
        if (rw->weight) l = rw->weight[i] * l;
        l = -l;
    }
    return l;
}

/* One step of the actor: pfs_step under pafs_rule. */
void pafs_step(const pfs_net *ac, pfs_opt *opt, const pfs_rows *rw, int n, const float *feat, const pfs_hyper *hp, float *grad_out,
               float *gfeat, float *out, float *status) {
    pfs_step(ac, opt, pafs_rule, rw, n, feat, hp, grad_out, gfeat, out, status);
}
