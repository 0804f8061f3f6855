// The Dreamer agent on the device (racecar_policy.hip), deterministic and sampled: what the C-ABI layer and the kernel share.
// Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RC_POLICY_STOCH 30
#define RC_POLICY_DETER 200
#define RC_POLICY_STATE (RC_POLICY_STOCH + RC_POLICY_DETER + 2)   // stoch | deter | raw previous action
#define RC_POLICY_UNITS 400                                       // actor width
#define RC_POLICY_TILE 32                                         // cars per workgroup = rows of one 32x32x2 MFMA tile
// Weight matrices are kept [K][ld] on the device with ld = the column count rounded up to whole 32-column tiles, the padding
// zero (weights and biases): a tile past the last output computes zeros that are never stored.  The GRU's two [200][600]
// matrices keep their three gates (z, r, candidate) at columns 0, 224 and 448 of ld = 672.
#define RC_POLICY_LD200 224
#define RC_POLICY_LD400 416
#define RC_POLICY_LDGRU (3 * RC_POLICY_LD200)
#define RC_POLICY_LDSMALL 32                                      // obs2 (30 mean columns), hout (2 mean columns)
// The sampled modes read obs2 and hout from images of their own at ld 64: the mean columns in tile 0, the std columns at the
// same offsets in tile 1, so that one wave holds mean and raw std of a (car, column) in matching accumulator registers.
#define RC_POLICY_LDPAIR 64

struct RcPolicyDev {
    const float *img1_w, *img1_b;            // [32][224], [224]
    const float *gru_k, *gru_r, *gru_b;      // [200][672] x 2, [2][672]
    const float *obs1_w, *obs1_b;            // [1280][224], [224]      rows: deter 200, then the 1080 beams
    const float *obs2_w, *obs2_b;            // [200][32], [32]         the 30 mean columns
    const float *h_w[4], *h_b[4];            // [230][416], 3 x [400][416]; [416]
    const float *hout_w, *hout_b;            // [400][32], [32]         the 2 mean columns
    const float *hnorm;                      // [4][2] mean, sqrt(var + eps), gamma, beta of the 2 mean columns; null = plain actor
};

struct RcPolicySampleDev {                   // what the sampled modes read on top
    const float *obs2_w, *obs2_b;            // [200][64], [64]         mean | std columns
    const float *hout_w, *hout_b;            // [400][64], [64]
    const float *hnorm4;                     // [4][4] mean, sqrt(var + eps), gamma, beta of all four output columns; null = plain actor
};

// The rows of a call and the key of their draws: row q is the car of env q / n_slots in the mask's (q % n_slots)-th slot; a car's
// draws are keyed by (first_env + env, episode, agent_steps, slot) under the seed ("random stream")
struct RcPolicyRows {
    int32_t n_active;                        // num_envs x (slots in the mask): the rows of this call
    int32_t cars_per_env, n_slots;
    uint32_t slots;                          // slot of the mask's k-th set bit in byte k
    uint32_t seed_lo, seed_hi, first_env;
    const uint32_t *episode;                 // [num_envs] the env's episode counter ...
    const int32_t *agent_steps;              // ... and its agent steps within the episode, as the last step or reset left them
};

struct RcPolicyCall {
    RcPolicyDev w;
    const float *lidar;                      // [n_cars][1080] metres
    const uint8_t *fresh;                    // [n_cars]
    float *state;                            // [n_cars][RC_POLICY_STATE]
    float *actions;                          // [n_cars][2] RC_F_ACTION_IN
    RcPolicyRows rows;                       // (the seed and the counters: the sampled modes only)
    int32_t raw_actions;                     // rc_config.remap_actions: the env maps [-1, 1]^2 itself
    float lo0, lo1, hi0, hi1;                // else: postprocess_action's range
    // the sampled modes only (rc_policy_set_sampling)
    int32_t mode;                            // RC_POLICY_MODE_DEPLOY | RC_POLICY_MODE_EXPLORE
    float expl_amount;
    RcPolicySampleDev ws;
};

// Imagination (racecar_imagine.hip): the prior's second half and the reward head, packed like the rest
struct RcImagineDev {
    const float *img2_w, *img2_b;            // [200][224], [224]
    const float *img3_w, *img3_b;            // [200][64], [64]         mean | std columns (mode `mean` reads tile 0 only); null = not loaded
    const float *rh_w[2], *rh_b[2];          // reward head [230][416], [400][416]; [416]; null = no heads loaded
    const float *rout_w, *rout_b;            // [400][32], [32]         its one output column
};

struct RcImagineCall {
    RcPolicyDev w;
    RcPolicySampleDev ws;
    RcImagineDev wi;
    const float *state;                      // [n_cars][RC_POLICY_STATE], read only
    RcPolicyRows rows;                       // (the draw's key: as rc_policy_act reads it)
    int32_t horizon, sample;
    const float *actions_in;                 // [n_cars][H][2] or null: the actor's own
    float *reward, *actions, *features, *reward_start;      // [n_cars][H], [n_cars][H][2], [n_cars][H][230], [n_cars]; any may be null
};

// Planning in the latent (racecar_dream.hip): rows are pairs (start, candidate), row = start x K + candidate
struct RcDreamCall {
    RcPolicyDev w;
    RcImagineDev wi;
    const float *state;                      // live: [n_cars][RC_POLICY_STATE] of the handle; else the caller's [starts][RC_POLICY_STATE]; read only
    RcPolicyRows rows;                       // live: start -> car (the caller's arrays are indexed by car)
    int32_t live;
    int32_t candidates;                      // K
    int64_t n_rows;                          // starts x K < 2^31 (live: the mask's cars x K)
    uint64_t row_offset;                     // not live: the start id of start 0; the draws are keyed by (start id, candidate, t)
    int32_t horizon, sample;
    uint32_t seed_lo, seed_hi;
    float discount;
    const float *actions_in;                 // [starts][K][H][2] raw
    float *ret, *reward, *final_feature;     // [starts][K], [starts][K][H], [starts][K][230]; any may be null
};

// The dream's backward pass (racecar_dream_grad.hip): the transposed weight images, [units above][units
// below rounded up to whole tiles], the padding zero - pm_gemm's B operand is coalesced backward as it is forward
#define RC_POLICY_LDT 256
struct RcDreamGradDev {
    const float *img1_t;                     // [200][32]
    const float *gruk_t, *grur_t;            // [600][256]: the gate units z, r, candidate one behind the other
    const float *img2_t;                     // [200][256]
    const float *img3_t;                     // [60][256]: the 30 mean units, then the 30 raw std units
    const float *rh0_t;                      // [400][256]: 230 columns, stoch | deter
    const float *rh1_t;                      // [400][416]
};

struct RcDreamGradCall {
    RcDreamCall d;                           // the forward's record; d.n_rows: the END of this launch's rows, d.final_feature unused
    RcDreamGradDev wt;
    int64_t row_begin;                       // the first row of this launch (a multiple of 32): workgroup b owns rows row_begin + 32 b ..
    float *stash;                            // [rows of the launch rounded up to 32][H][RC_DREAM_GRAD_STASH]
    float *grad_actions, *grad_state;        // [starts][K][H][2], [starts][K][230]; any may be null
};

// The critic (racecar_returns.hip): the value head and the optional pcont head, DenseDecoder((), 3, 400)
// each, packed like the reward head
struct RcCriticDev {
    const float *vh_w[3], *vh_b[3];          // value head [230][416], 2 x [400][416]; [416]; null = no critic loaded
    const float *vout_w, *vout_b;            // [400][32], [32]         its one output column
    const float *ph_w[3], *ph_b[3];          // pcont head, the same shapes; null = none (a constant pcont)
    const float *pout_w, *pout_b;
};

// Rows are starts: the cars of the mask (live: arrays indexed by car) or the rows of a given state
struct RcReturnsCall {
    RcPolicyDev w;
    RcPolicySampleDev ws;
    RcImagineDev wi;
    RcCriticDev wc;
    const float *state;                      // live: [n_cars][RC_POLICY_STATE] of the handle; else the caller's [starts][RC_POLICY_STATE]; read only
    RcPolicyRows rows;                       // live: row -> car, and the key of its draws (rc_policy_imagine's)
    int32_t live;
    int64_t n_rows;                          // < 2^31
    uint64_t row_offset;                     // not live: the id of row 0; the draws are keyed by (row id, t)
    int32_t horizon, sample;
    uint32_t seed_lo, seed_hi;               // (not live)
    float lambda, discount;
    const float *actions_in;                 // [rows][H][2] raw, or null: the actor's own
    float *reward, *value, *pcont;           // [rows][H]; any output may be null
    float *returns, *weight;                 // [rows][H - 1]
    float *actions, *features;               // [rows][H][2], [rows][H][230]
    float *reward_start, *value_start, *pcont_start;      // [rows]
};

// The actor loss's gradient through the dream (racecar_returns_grad.hip): rc_policy_dream_grad's transposed
// images and the critic's, in the same two shapes ([400][256] for a first layer's 230 columns, [400][416] for a hidden layer)
struct RcReturnsGradDev {
    RcDreamGradDev p;                        // the prior's five and the reward head's two
    const float *vh_t[3];                    // value head: [400][256], 2 x [400][416]
    const float *ph_t[3];                    // pcont head, the same shapes; null = none loaded
};

struct RcReturnsGradCall {
    RcReturnsCall r;                         // the forward's record; r.n_rows: the END of this launch's rows
    RcReturnsGradDev wt;
    int64_t row_begin;                       // the first row of this launch (a multiple of 32): workgroup b owns rows row_begin + 32 b ..
    float *stash;                            // [rows of the launch rounded up to 32][H][RC_RETURNS_GRAD_STASH]
    float scale;
    float *grad_actions, *actor_features, *eps, *grad_state;      // [rows][H][2], [rows][H][230], [rows][H][2], [rows][230]; any may be null
};

// Recorded sequences (racecar_observe.hip): rows are windows [T] of scans and actions, not cars of the env
struct RcObserveCall {
    RcPolicyDev w;
    RcPolicySampleDev ws;                    // (obs2's pair image: both modes)
    RcImagineDev wi;
    int64_t rows;
    uint64_t row_offset;                     // row id of row 0: the draws are keyed by (row id, t)
    int32_t length, context, sample;
    uint32_t seed_lo, seed_hi;
    const float *scan;                       // [rows][T][1080] metres
    const float *actions;                    // [rows][T][2] raw
    const float *state_in;                   // [rows][RC_POLICY_STATE] or null: zeros
    float *features, *post_mean, *post_std, *prior_mean, *prior_std;      // [rows][T][230] / [rows][T][30]; any may be null
    float *kl, *reward;                      // [rows][T]
    float *state_out;                        // [rows][RC_POLICY_STATE]
};

// The observation decoder (racecar_decode.hip): the LidarOccupancyDecoder's arrays, each repacked for the
// order in which its kernel reads it (u, v kernel row and column, c input channel, o output channel; a 6 x 6 kernel's tap is
// (ty, tx) with u = py + 2 ty, v = px + 2 tx for the output's parity class (py, px))
#define RC_DEC_H1 64
#define RC_DEC_H2 800                                             // 5 x 5 x 32
struct RcDecodeDev {
    const float *h1_w, *h1_b;                // [230][64], [64]
    const float *h2_k, *h2_b;                // [c 64][(u 5 + v) 32 + o], [32]
    const float *h3_k, *h3_b;                // [o / 4][u][v][c 32][o % 4], [16]
    const float *h4_k, *h4_b;                // [ty][tx][c 16][py][px][o 8], [8]
    const float *h5_k, *h5_b;                // [ty][tx][c 8][py][px], [1]
};

struct RcDecodeCall {
    RcDecodeDev w;
    const float *features;                   // [n_rows][230], or null: the rows of `rows` from state
    const float *state;                      // [n_cars][RC_POLICY_STATE], read only
    RcPolicyRows rows;                       // (live latents: row -> car; outputs are indexed by car)
    int64_t n_rows;
    float *logits;                           // [..][64][64] or null
    uint8_t *image;                          // [..][64][64] or null
    int32_t *mismatch;                       // [n_cars] or null
    const uint8_t *occupancy;                // RC_F_OCCUPANCY [n_cars][64][64] (mismatch only)
};

// The LiDAR distance decoder (racecar_decode_lidar.hip): LidarDistanceDecoder's three dense layers.  The
// last layer's image is padded so that every 32-column tile of a (loc, scale) pair lies inside it: loc columns at [0, 1080),
// scale columns at [RC_LDEC_HALF, RC_LDEC_HALF + 1080), the rest zero (weights and bias).
#define RC_LDEC_H1 256
#define RC_LDEC_H2 512
#define RC_LDEC_BEAMS 1080
#define RC_LDEC_HALF 1088                                         // 34 tiles
#define RC_LDEC_LD (2 * RC_LDEC_HALF)
struct RcLidarDecodeDev {
    const float *d1_w, *d1_b;                // [230][256], [256]
    const float *d2_w, *d2_b;                // [256][512], [512]
    const float *p_w, *p_b;                  // [512][2176], [2176]
};

struct RcLidarDecodeCall {
    RcLidarDecodeDev w;
    const float *features;                   // [n_rows][230], or null: the rows of `rows` from state
    const float *state;                      // [n_cars][RC_POLICY_STATE], read only
    RcPolicyRows rows;                       // (live latents: row -> car; outputs and the target are indexed by car)
    int64_t n_rows;
    const float *target;                     // [..][1080] metres (loglik only): the caller's, or the arena's RC_F_LIDAR
    float *mean, *std;                       // [..][1080] or null
    float *loglik;                           // [..] or null
};

// The same decoder with the Bernoulli log-likelihood of a target image (rc_policy_decode_loglik)
struct RcDecodeLoglikCall {
    RcDecodeCall d;
    const uint8_t *target;                   // [..][64][64], indexed as the outputs are (loglik only): the caller's, or RC_F_OCCUPANCY
    float *loglik;                           // [..] or null
};

hipError_t rck_policy_prepare();             // raises the kernel's dynamic-LDS limit (once per process and device is enough)
hipError_t rck_launch_policy(const RcPolicyCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);      // c.mode: which kernel
hipError_t rck_imagine_prepare();
hipError_t rck_launch_imagine(const RcImagineCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);                // c.sample: which kernel
hipError_t rck_dream_prepare();
hipError_t rck_launch_dream(const RcDreamCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);                    // c.sample: which kernel
hipError_t rck_dream_grad_prepare();
hipError_t rck_returns_grad_prepare();
hipError_t rck_observe_prepare();
hipError_t rck_launch_observe(const RcObserveCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);                // c.sample: which kernel
hipError_t rck_returns_prepare();
hipError_t rck_launch_returns(const RcReturnsCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);                // c.sample: which kernel
hipError_t rck_decode_prepare();
hipError_t rck_launch_decode(const RcDecodeCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);
hipError_t rck_launch_decode_loglik(const RcDecodeLoglikCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);      // (rck_decode_prepare covers it)
hipError_t rck_decode_lidar_prepare();
hipError_t rck_launch_decode_lidar(const RcLidarDecodeCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s);
