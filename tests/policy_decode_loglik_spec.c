/* The binary32 specification of the observation decoder's Bernoulli log-likelihood (rc_policy_decode_loglik;
 * Independent(Bernoulli(logits), 3).log_prob of dreamer/models.py:464), for the CPU under the conventions of policy_spec.c; built
 * with -ffp-contract=off -fno-fast-math by tests/policy_decode_loglik_spec.py.  The logits are those of policy_decode_spec.c; this
 * file restates the epilogue of racing_dreamer_amd/csrc/racecar_decode.hip's second instantiation and includes nothing of it;
 * softplus is policy_sample_spec.c's.
 *
 * term(y, x) = (target[y][x] != 0 ? logit[y][x] : 0.0f) - softplus(logit[y][x]).
 * Order of summation: 512 threads; thread t owns the 2 x 2 pixel blocks `item` = t and t + 512, block (Y, X) = (item / 32,
 * item % 32) holding pixels (2 Y + py, 2 X + px).  A thread adds its 8 terms from +0.0f in the order item, py, px.  The 64 threads
 * of wave t / 64 are added in a binary tree over t % 64 (neighbours at distance 1, then 2, 4, 8, 16, 32); the 8 wave sums are added
 * in ascending order from +0.0f. */
#include "policy_sample_spec.c"

#define PDL_IMG 64

void pdl_loglik(int n, const float *logits, const uint8_t *target, float *out) {
    for (int i = 0; i < n; ++i) {
        const float *lg = logits + (size_t)i * PDL_IMG * PDL_IMG;
        const uint8_t *tg = target + (size_t)i * PDL_IMG * PDL_IMG;
        float total = 0.0f;
        for (int wave = 0; wave < 8; ++wave) {
            float v[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int t = 64 * wave + lane;
                float s = 0.0f;
                for (int k = 0; k < 2; ++k) {
                    const int item = t + 512 * k, Y = item >> 5, X = item & 31;
                    for (int py = 0; py < 2; ++py)
                        for (int px = 0; px < 2; ++px) {
                            const int p = (2 * Y + py) * PDL_IMG + 2 * X + px;
                            s = s + ((tg[p] ? lg[p] : 0.0f) - pss_softplus(lg[p]));
                        }
                }
                v[lane] = s;
            }
            for (int m = 1; m < 64; m <<= 1)
                for (int j = 0; j < 64; j += 2 * m) v[j] = v[j] + v[j + m];
            total = total + v[0];
        }
        out[i] = total;
    }
}
