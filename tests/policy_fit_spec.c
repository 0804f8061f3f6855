/* The binary32 specification of the critic's fit (rc_policy_fit_step), restated for the CPU under the
 * conventions of policy_spec.c (plain C11, one IEEE operation per written operator, fmaf where a fused operation is meant; built
 * with -O2 -ffp-contract=off -fno-fast-math by tests/policy_fit_spec.py).  It includes policy_returns_spec.c - and through it the
 * other specs - unchanged for ps_dense, ps_elu, ps_sigmoid and pss_softplus, and restates racing_dreamer_amd/csrc/racecar_fit.hip; it
 * includes nothing of it.  The arithmetic is the reference's value update, dreamer/models.py:129-137 (value_loss under value_opt, the
 * targets stop_gradient(returns)) and dreamer/tools.py:421-455 (`Optimizer`: clip_by_global_norm, then Adam = TF's ResourceApplyAdam),
 * and for the pcont head the Bernoulli likelihood of models.py:101-105 on soft targets.
 *
 * One step on N rows (features [N][230] = stoch | deter, target [N], weight [N] or NULL = all 1):
 *   forward    a0 = the features; a_{l+1} = elu(a_l W_l + b_l), l = 0, 1, 2, and o = a3 Wout + bout: bias first, then the
 *              k-ascending fmaf chain (ps_dense), then ps_elu - policy_returns_spec.c's prs_head3 with the activations kept.
 *   loss term  value: e = o - t, lp = fmaf(-0.5, e e, -log(2 pi) / 2);  pcont: lp = -fmaf(t, softplus(-o), (1 - t) softplus(o)),
 *              e = sigmoid(o) - t;  with a weight both are multiplied by it: e = w e, lp = w lp.
 *   delta_o    = e inv_n, inv_n = 1.0f / (float)N computed once.
 *   backward   delta3 = fmaf(delta_o, Wout[j], 0) elu'(a3[j]); delta2 = (delta3 W2^T) elu'(a2); delta1 = (delta2 W1^T) elu'(a1);
 *              every product a k-ascending fmaf chain FROM ZERO over the 400 units above; elu'(a) = a > 0 ? 1 : a + 1 from the
 *              stored activation.  No gradient with respect to the features.
 *   gradients  G_l = [a_{l-1} | 1]^T delta_l, [K_l + 1][400] (the last row is the bias gradient), G_out [401][1]: the eight arrays of
 *              the head one behind the other, 413 601 floats.  THE ORDER OF THE ROW SUM: row r belongs to chain (r / 2) mod 4; a
 *              chain is c = fmaf(a[r][k], delta[r][j], c) from zero over its rows in ascending order; G = (c0 + c1) + (c2 + c3).
 *   sums       pfs_tree: the sum of n binary32 numbers in binary64 - element i belongs to slot i mod 32 768, a slot adds its
 *              elements in ascending order, every group of 256 consecutive slots halves seven times (s[t] += s[t + stride], stride
 *              128 .. 1), the 128 group sums are added in ascending order.  norm = (float)sqrt(tree of the binary32 squares g g);
 *              loss = (float)(-(tree of the loss terms / (double)N)).
 *   skip       norm not finite: nothing changes, the step does not count, skipped = 1 (the reference's LossScaleOptimizer; the
 *              loss scale itself, a power of two under precision 32, is not modelled).
 *   clip       scale = clip > 0 ? clip / max(norm, clip) : 1;  g = g scale (norm <= clip: scale is exactly 1).
 *   Adam       step += 1; b1pow *= beta1, b2pow *= beta2 (binary64 running products);  c1 = (float)(1 - b1pow), c2 likewise;
 *              lr_t = (lr sqrtf(c2)) / c1;  m = fmaf(beta1, m, (1 - beta1) g);  v = fmaf(beta2, v, (1 - beta2) (g g));
 *              w = fmaf(-lr_t, m / (sqrtf(v) + epsilon), w).  No weight decay (0 in the reference's config). */
#include "policy_returns_spec.c"
#include <stdlib.h>

#define PFS_FEAT 230
#define PFS_UNITS 400
#define PFS_G1 ((PFS_FEAT + 1) * PFS_UNITS)
#define PFS_G2 (PFS_G1 + (PFS_UNITS + 1) * PFS_UNITS)
#define PFS_GO (PFS_G2 + (PFS_UNITS + 1) * PFS_UNITS)
#define PFS_NG (PFS_GO + PFS_UNITS + 1)             /* 413 601 */
#define PFS_GROUPS 128
#define PFS_GROUP 256

typedef struct pfs_head {
    float *h_w[3], *h_b[3], *out_w, *out_b;         /* the checkpoint's arrays, row-major, updated in place */
} pfs_head;

typedef struct pfs_opt {
    float *m, *v;                                   /* [PFS_NG] each, in the order of the gradient */
    double b1pow, b2pow;
    int32_t step;
} pfs_opt;

typedef struct pfs_hyper { float lr, clip, beta1, beta2, epsilon; } pfs_hyper;

int pfs_grad_size(void) { return PFS_NG; }

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

/* The forward and backward pass: grad [PFS_NG] (before the clip), lterm [n].  kind 0: the value head, 1: the pcont head. */
void pfs_gradient(const pfs_head *hd, int kind, int n, const float *feat, const float *target, const float *weight, float *grad, float *lterm) {
    const size_t plane = (size_t)n * PFS_UNITS;
    float *buf = (float *)malloc((6 * plane + (size_t)n) * sizeof(float));
    float *chains = (float *)malloc((size_t)4 * (PFS_UNITS + 1) * PFS_UNITS * sizeof(float));
    float *a1 = buf, *a2 = buf + plane, *a3 = buf + 2 * plane, *d1 = buf + 3 * plane, *d2 = buf + 4 * plane, *d3 = buf + 5 * plane;
    float *dout = buf + 6 * plane;
    const float inv_n = 1.0f / (float)n;
    for (int i = 0; i < n; ++i) {
        float *x1 = a1 + (size_t)i * PFS_UNITS, *x2 = a2 + (size_t)i * PFS_UNITS, *x3 = a3 + (size_t)i * PFS_UNITS, o, tmp[PFS_UNITS];
        ps_dense(feat + (size_t)i * PFS_FEAT, PFS_FEAT, hd->h_w[0], 400, 0, hd->h_b[0], 400, x1);
        for (int j = 0; j < 400; ++j) x1[j] = ps_elu(x1[j]);
        ps_dense(x1, 400, hd->h_w[1], 400, 0, hd->h_b[1], 400, x2);
        for (int j = 0; j < 400; ++j) x2[j] = ps_elu(x2[j]);
        ps_dense(x2, 400, hd->h_w[2], 400, 0, hd->h_b[2], 400, x3);
        for (int j = 0; j < 400; ++j) x3[j] = ps_elu(x3[j]);
        ps_dense(x3, 400, hd->out_w, 1, 0, hd->out_b, 1, &o);
        const float t = target[i];
        float e, lp;
        if (kind == 1) {
            lp = -fmaf(t, pss_softplus(-o), (1.0f - t) * pss_softplus(o));
            e = ps_sigmoid(o) - t;
        } else {
            e = o - t;
            lp = fmaf(-0.5f, e * e, -0.9189385332f);
        }
        if (weight) {
            e = weight[i] * e;
            lp = weight[i] * lp;
        }
        const float delta = e * inv_n;
        dout[i] = delta;
        lterm[i] = lp;
        float *g3 = d3 + (size_t)i * PFS_UNITS, *g2 = d2 + (size_t)i * PFS_UNITS, *g1 = d1 + (size_t)i * PFS_UNITS;
        for (int j = 0; j < 400; ++j) g3[j] = fmaf(delta, hd->out_w[j], 0.0f) * pfs_elu_grad(x3[j]);
        pfs_back(g3, hd->h_w[2], 400, tmp);
        for (int j = 0; j < 400; ++j) g2[j] = tmp[j] * pfs_elu_grad(x2[j]);
        pfs_back(g2, hd->h_w[1], 400, tmp);
        for (int j = 0; j < 400; ++j) g1[j] = tmp[j] * pfs_elu_grad(x1[j]);
    }
    pfs_wgrad(n, feat, PFS_FEAT, PFS_FEAT, d1, PFS_UNITS, PFS_UNITS, chains, grad);
    pfs_wgrad(n, a1, PFS_UNITS, PFS_UNITS, d2, PFS_UNITS, PFS_UNITS, chains, grad + PFS_G1);
    pfs_wgrad(n, a2, PFS_UNITS, PFS_UNITS, d3, PFS_UNITS, PFS_UNITS, chains, grad + PFS_G2);
    pfs_wgrad(n, a3, PFS_UNITS, PFS_UNITS, dout, 1, 1, chains, grad + PFS_GO);
    free(chains);
    free(buf);
}

/* the weight behind gradient element e */
static float *pfs_weight(const pfs_head *hd, int e) {
    if (e >= PFS_GO) return e - PFS_GO < PFS_UNITS ? hd->out_w + (e - PFS_GO) : hd->out_b;
    const int l = e < PFS_G1 ? 0 : (e < PFS_G2 ? 1 : 2);
    const int i = e - (l == 0 ? 0 : (l == 1 ? PFS_G1 : PFS_G2)), K = l == 0 ? PFS_FEAT : PFS_UNITS;
    return i < K * PFS_UNITS ? hd->h_w[l] + i : hd->h_b[l] + (i - K * PFS_UNITS);
}

/* One step.  grad_out [PFS_NG] or NULL: the gradient before the clip.  status [4] = loss, grad_norm, skipped, step. */
void pfs_step(const pfs_head *hd, pfs_opt *opt, int kind, int n, const float *feat, const float *target, const float *weight, const pfs_hyper *hp,
              float *grad_out, float *status) {
    float *grad = (float *)malloc((size_t)PFS_NG * sizeof(float)), *lterm = (float *)malloc((size_t)n * sizeof(float));
    pfs_gradient(hd, kind, n, feat, target, weight, grad, lterm);
    if (grad_out) memcpy(grad_out, grad, (size_t)PFS_NG * sizeof(float));
    const float norm = (float)sqrt(pfs_tree(grad, PFS_NG, 1));
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
        for (int e = 0; e < PFS_NG; ++e) {
            float *w = pfs_weight(hd, e);
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
