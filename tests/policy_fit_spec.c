/* The binary32 specification of the fit engine (rc_policy_fit_step for the critic's two heads and -
 * with RC_POLICY_FIT_REWARD - the reward head, rc_policy_actor_fit_step for the actor), restated for the CPU under the conventions of
 * policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is meant; built with -O2
 * -ffp-contract=off -fno-fast-math by tests/policy_fit_spec.py).  It includes policy_returns_spec.c - and through it the other specs -
 * unchanged for ps_dense, ps_elu, ps_sigmoid and pss_softplus, and restates racing_dreamer_amd/csrc/racecar_fit.hip; it includes
 * nothing of it.  As the device has one fit_rows<DEPTH, FORWARD_ONLY>, this is ONE engine over a network of `depth` hidden layers of
 * 400 on 230 features with `n_out` outputs, and a per-row output rule; policy_actor_fit_spec.c puts the actor's rule on top of it.
 * The optimizer is the reference's dreamer/tools.py:421-455 (`Optimizer`: clip_by_global_norm, then Adam = TF's ResourceApplyAdam).
 *
 * One step on N rows (features [N][230] = stoch | deter, the rule's rows in pfs_rows), D = depth, W = n_out:
 *   forward    a0 = the features; a_{l+1} = elu(a_l W_l + b_l), l = 0 .. D - 1, and o [W] = a_D Wout + bout: bias first, then the
 *              k-ascending fmaf chain (ps_dense), then ps_elu - policy_returns_spec.c's prs_head3 with the activations kept.
 *   rule       o [W] -> delta o [W] and the row's stored loss term, inv_n = 1.0f / (float)N computed once (below, and the actor's).
 *   backward   delta_D[j] = (the fmaf chain FROM +0 over c = 0 .. W - 1 of delta o_c Wout[j][c]) elu'(a_D[j]) - at W = 1
 *              fmaf(delta_o, Wout[j], 0) -; delta_l = (delta_{l+1} W_l^T) elu'(a_l), l = D - 1 .. 1; every product a k-ascending
 *              fmaf chain FROM ZERO over the 400 units above (pfs_back); elu'(a) = a > 0 ? 1 : a + 1 from the stored activation.
 *              grad_features, where asked for, = delta_1 W_0^T, the same chain.
 *   gradients  G_l = [a_l | 1]^T delta_{l+1}, [K_l + 1][400] (the last row is the bias gradient), G_out [401][W]: the 2 D + 2 arrays
 *              of the network one behind the other, [231][400] | (D - 1) x [401][400] | [401][W] floats.  THE ORDER OF THE ROW SUM:
 *              row r belongs to chain (r / 2) mod 4; a chain is c = fmaf(a[r][k], delta[r][j], c) from zero over its rows in ascending
 *              order; G = (c0 + c1) + (c2 + c3).
 *   sums       pfs_tree: the sum of n binary32 numbers in binary64 - element i belongs to slot i mod 32 768, a slot adds its
 *              elements in ascending order, every group of 256 consecutive slots halves seven times (s[t] += s[t + stride], stride
 *              128 .. 1), the 128 group sums are added in ascending order.  norm = (float)sqrt(tree of the binary32 squares g g);
 *              loss = (float)(-(tree of the loss terms / (double)N)).
 *   skip       norm not finite: nothing changes, the step does not count, skipped = 1 (the reference's LossScaleOptimizer; the
 *              loss scale itself, a power of two under precision 32, is not modelled).
 *   clip       scale = clip > 0 ? clip / max(norm, clip) : 1;  g = g scale (norm <= clip: scale is exactly 1).
 *   Adam       step += 1; b1pow *= beta1, b2pow *= beta2 (binary64 running products);  c1 = (float)(1 - b1pow), c2 likewise;
 *              lr_t = (lr sqrtf(c2)) / c1;  m = fmaf(beta1, m, (1 - beta1) g);  v = fmaf(beta2, v, (1 - beta2) (g g));
 *              w = fmaf(-lr_t, m / (sqrtf(v) + epsilon), w).  No weight decay (0 in the reference's config).
 *
 * What the depth and the rule change per head:
 *   value      D = 3, W = 1, 413 601 floats; Normal(o, 1) against stop_gradient(returns), the reference's value update
 *              (dreamer/models.py:129-137, value_loss under value_opt): e = o - t, lp = fmaf(-0.5, e e, -log(2 pi) / 2).
 *   pcont      D = 3, W = 1; the Bernoulli likelihood of models.py:101-105 on soft targets:
 *              lp = -fmaf(t, softplus(-o), (1 - t) softplus(o)), e = sigmoid(o) - t.
 *   reward     D = 2, W = 1, 253 201 floats; the reference's DenseDecoder((), 2, 400) (models.py:167) under Normal(o, 1) against the
 *              recorded reward (models.py:97-100): the value head's rule.
 *   all three  with a weight both are multiplied by it: e = w e, lp = w lp; then delta o = e inv_n.
 *   actor      D = 4, W = 4, 575 204 floats: policy_actor_fit_spec.c. */
#include "policy_returns_spec.c"
#include <stdlib.h>

#define PFS_FEAT 230
#define PFS_UNITS 400
#define PFS_G1 ((PFS_FEAT + 1) * PFS_UNITS)
#define PFS_GL ((PFS_UNITS + 1) * PFS_UNITS)
#define PFS_MAX_DEPTH 4
#define PFS_MAX_OUT 4
#define PFS_GROUPS 128
#define PFS_GROUP 256

typedef struct pfs_net {
    int32_t depth, n_out;                           /* 2, 3 or 4 hidden layers; 1 or 4 outputs */
    float *h_w[PFS_MAX_DEPTH], *h_b[PFS_MAX_DEPTH], *out_w, *out_b;      /* the checkpoint's arrays, row-major, updated in place */
} pfs_net;

typedef struct pfs_rows {                           /* what the rules read, [n] or [n][2] each; NULL where a rule takes none */
    int32_t kind;                                   /* 0: Normal(o, 1), 1: Bernoulli (the actor's rule does not read it) */
    const float *target, *weight, *eps, *grad;
} pfs_rows;

/* o [n_out] of row i -> delta_o [n_out]; returns the row's stored loss term */
typedef float (*pfs_rule)(const pfs_rows *rw, int i, float inv_n, const float *o, float *delta_o);

typedef struct pfs_opt {
    float *m, *v;                                   /* [pfs_grad_size] each, in the order of the gradient */
    double b1pow, b2pow;
    int32_t step;
} pfs_opt;

typedef struct pfs_hyper { float lr, clip, beta1, beta2, epsilon; } pfs_hyper;

/* where hidden layer l's [K_l + 1][400] begins in the gradient; l = depth: the output layer's [401][n_out] */
static int pfs_layer_at(int l) { return l == 0 ? 0 : PFS_G1 + (l - 1) * PFS_GL; }

int pfs_grad_size(const pfs_net *nt) { return pfs_layer_at(nt->depth) + (PFS_UNITS + 1) * nt->n_out; }

/* the fixed tree: x [n] binary32 (square: its binary32 squares) summed in binary64 */
double pfs_tree(const float *x, int64_t n, int square) {
    double total = 0.0;
    for (int b = 0; b < PFS_GROUPS; ++b) {
        double s[PFS_GROUP];
        for (int t = 0; t < PFS_GROUP; ++t) {
            double acc = 0.0;
            for (int64_t i = (int64_t)b * PFS_GROUP + t; i < n; i += PFS_GROUPS * PFS_GROUP) {
                const float q = square ? x[i] * x[i] : x[i];
                acc += (double)q;
            }
            s[t] = acc;
        }
        for (int stride = PFS_GROUP / 2; stride >= 1; stride >>= 1)
            for (int t = 0; t < stride; ++t) s[t] += s[t + stride];
        total += s[0];
    }
    return total;
}

static float pfs_elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }

/* out[i] = sum over j ascending of fmaf(delta[j], w[i][j], .) from zero, i < n_in: delta W^T for one row */
static void pfs_back(const float *delta, const float *w, int n_in, float *out) {
    for (int i = 0; i < n_in; ++i) {
        float acc = 0.0f;
        const float *row = w + (size_t)i * PFS_UNITS;
        for (int j = 0; j < PFS_UNITS; ++j) acc = fmaf(delta[j], row[j], acc);
        out[i] = acc;
    }
}

/* G [K + 1][nc] = [a | 1]^T delta over the rows, in the four chains; chains: [4][K + 1][nc] of scratch */
static void pfs_wgrad(int n, const float *a, int lda, int K, const float *delta, int ldd, int nc, float *chains, float *G) {
    const size_t size = (size_t)(K + 1) * nc;
    for (size_t i = 0; i < 4 * size; ++i) chains[i] = 0.0f;
    for (int r = 0; r < n; ++r) {
        float *c = chains + (size_t)((r / 2) % 4) * size;
        const float *ar = a + (size_t)r * lda, *dr = delta + (size_t)r * ldd;
        for (int k = 0; k <= K; ++k) {
            const float ak = k < K ? ar[k] : 1.0f;
            float *ck = c + (size_t)k * nc;
            for (int j = 0; j < nc; ++j) ck[j] = fmaf(ak, dr[j], ck[j]);
        }
    }
    for (size_t i = 0; i < size; ++i) G[i] = (chains[i] + chains[size + i]) + (chains[2 * size + i] + chains[3 * size + i]);
}

/* the forward pass of one row: a[l] [400] = a_{l+1}, l < depth; o [n_out] */
static void pfs_forward_row(const pfs_net *nt, const float *feat, float *const *a, float *o) {
    const float *x = feat;
    for (int l = 0; l < nt->depth; ++l) {
        ps_dense(x, l ? PFS_UNITS : PFS_FEAT, nt->h_w[l], 400, 0, nt->h_b[l], 400, a[l]);
        for (int j = 0; j < 400; ++j) a[l][j] = ps_elu(a[l][j]);
        x = a[l];
    }
    ps_dense(x, 400, nt->out_w, nt->n_out, 0, nt->out_b, nt->n_out, o);
}

/* the rule of the value, reward (kind 0) and pcont (kind 1) heads */
static float pfs_likelihood(const pfs_rows *rw, int i, float inv_n, const float *o, float *delta_o) {
    const float t = rw->target[i];
    float e, lp;
    if (rw->kind == 1) {
        lp = -fmaf(t, pss_softplus(-*o), (1.0f - t) * pss_softplus(*o));
        e = ps_sigmoid(*o) - t;
    } else {
        e = *o - t;
        lp = fmaf(-0.5f, e * e, -0.9189385332f);
    }
    if (rw->weight) {
        e = rw->weight[i] * e;
        lp = rw->weight[i] * lp;
    }
    *delta_o = e * inv_n;
    return lp;
}

/* The forward and backward pass: grad [pfs_grad_size] (before the clip), lterm [n], gfeat [n][230] or NULL, out [n][n_out] or NULL
 * (the output layer's o). */
static void pfs_gradient(const pfs_net *nt, pfs_rule rule, const pfs_rows *rw, int n, const float *feat, float *grad, float *lterm,
                         float *gfeat, float *out) {
    const int D = nt->depth, W = nt->n_out;
    const size_t plane = (size_t)n * PFS_UNITS;
    float *buf = (float *)malloc((2 * D * plane + (size_t)n * W) * sizeof(float));
    float *chains = (float *)malloc((size_t)4 * (PFS_UNITS + 1) * PFS_UNITS * sizeof(float));
    float *a[PFS_MAX_DEPTH], *d[PFS_MAX_DEPTH], *dout = buf + 2 * D * plane;        /* a[l]: a_{l+1}; d[l]: delta_{l+1} */
    for (int l = 0; l < D; ++l) {
        a[l] = buf + (size_t)l * plane;
        d[l] = buf + (size_t)(D + l) * plane;
    }
    const float inv_n = 1.0f / (float)n;
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)i * PFS_UNITS;
        float o[PFS_MAX_OUT], tmp[PFS_UNITS], *row[PFS_MAX_DEPTH], *dq = dout + (size_t)i * W;
        for (int l = 0; l < D; ++l) row[l] = a[l] + at;
        pfs_forward_row(nt, feat + (size_t)i * PFS_FEAT, row, o);
        const float *x = row[D - 1];
        if (out) memcpy(out + (size_t)i * W, o, (size_t)W * sizeof(float));
        lterm[i] = rule(rw, i, inv_n, o, dq);
        float *g = d[D - 1] + at;
        for (int j = 0; j < 400; ++j) {
            const float *wr = nt->out_w + (size_t)j * W;
            float s = 0.0f;
            for (int c = 0; c < W; ++c) s = fmaf(dq[c], wr[c], s);
            g[j] = s * pfs_elu_grad(x[j]);
        }
        for (int l = D - 2; l >= 0; --l) {                                 /* delta_{l+1} from delta_{l+2} through W_{l+1}^T */
            pfs_back(d[l + 1] + at, nt->h_w[l + 1], 400, tmp);
            g = d[l] + at;
            for (int j = 0; j < 400; ++j) g[j] = tmp[j] * pfs_elu_grad(row[l][j]);
        }
        if (gfeat) pfs_back(d[0] + at, nt->h_w[0], PFS_FEAT, gfeat + (size_t)i * PFS_FEAT);
    }
    pfs_wgrad(n, feat, PFS_FEAT, PFS_FEAT, d[0], PFS_UNITS, PFS_UNITS, chains, grad);
    for (int l = 1; l < D; ++l) pfs_wgrad(n, a[l - 1], PFS_UNITS, PFS_UNITS, d[l], PFS_UNITS, PFS_UNITS, chains, grad + pfs_layer_at(l));
    pfs_wgrad(n, a[D - 1], PFS_UNITS, PFS_UNITS, dout, W, W, chains, grad + pfs_layer_at(D));
    free(chains);
    free(buf);
}

/* the weight behind gradient element e */
static float *pfs_weight(const pfs_net *nt, int e) {
    const int go = pfs_layer_at(nt->depth), wo = PFS_UNITS * nt->n_out;
    if (e >= go) return e - go < wo ? nt->out_w + (e - go) : nt->out_b + (e - go - wo);
    const int l = e < PFS_G1 ? 0 : 1 + (e - PFS_G1) / PFS_GL;
    const int i = e - pfs_layer_at(l), K = l == 0 ? PFS_FEAT : PFS_UNITS;
    return i < K * PFS_UNITS ? nt->h_w[l] + i : nt->h_b[l] + (i - K * PFS_UNITS);
}

/* One step under `rule`.  grad_out [pfs_grad_size] or NULL: the gradient before the clip; gfeat [n][230] or NULL; out [n][n_out] or
 * NULL.  status [4] = loss, grad_norm, skipped, step. */
static void pfs_step(const pfs_net *nt, pfs_opt *opt, pfs_rule rule, const pfs_rows *rw, int n, const float *feat, const pfs_hyper *hp,
                     float *grad_out, float *gfeat, float *out, float *status) {
    const int ng = pfs_grad_size(nt);
    float *grad = (float *)malloc((size_t)ng * sizeof(float)), *lterm = (float *)malloc((size_t)n * sizeof(float));
    pfs_gradient(nt, rule, rw, n, feat, grad, lterm, gfeat, out);
    if (grad_out) memcpy(grad_out, grad, (size_t)ng * sizeof(float));
    const float norm = (float)sqrt(pfs_tree(grad, ng, 1));
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
        for (int e = 0; e < ng; ++e) {
            float *w = pfs_weight(nt, e);
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

/* One step of a head with one output under Normal(o, 1) or the Bernoulli likelihood: rw->target [n], rw->weight [n] or NULL. */
void pfs_head_step(const pfs_net *nt, pfs_opt *opt, const pfs_rows *rw, int n, const float *feat, const pfs_hyper *hp, float *grad_out,
                   float *gfeat, float *out, float *status) {
    pfs_step(nt, opt, pfs_likelihood, rw, n, feat, hp, grad_out, gfeat, out, status);
}
