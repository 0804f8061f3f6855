/*
 * racecar_hip.h - C ABI of libracecar_hip.so: the MI355X (gfx950) batched F1TENTH racing
 * environment.  Plain C, plain pointers and sizes; no torch / C++ types cross this boundary.
 *
 * What this replaces in the reference (CPS-TUWien/racing_dreamer).  The reference has no
 * native code; its "FFI" for this path is the Python call into the external simulator
 * `racecar_gym` (PyBullet).  Each entry point below cites the reference call site whose
 * role it takes over:
 *
 *   rc_create / rc_load_track ... MultiAgentScenario.from_spec + MultiAgentRaceEnv(scenario)
 *                                 dreamer/wrappers.py:14-15;  SingleAgentScenario.from_spec +
 *                                 ChangingTrackSingleAgentRaceEnv(...)
 *                                 baselines/racing/experiments/sb3/sb_experiment.py:61-63
 *   rc_reset .................... env.reset(mode='grid'|'random'|'random_ball')
 *                                 dreamer/wrappers.py:72,91-92; baselines/racing/environment/common.py:28-29
 *   rc_step ..................... env.step({'A': {'motor', 'steering'}})   dreamer/wrappers.py:62-64
 *                                 with ActionRepeat (wrappers.py:107-116), ReduceActionSpace
 *                                 (wrappers.py:128-134) and TimeLimit (wrappers.py:147-154) folded in
 *   rc_get / rc_copy_out ........ the obs / reward / done / info dicts returned by step()
 *                                 dreamer/wrappers.py:64-69,210-226
 *   RC_F_OCCUPANCY .............. OccupancyMapObs.step                     dreamer/wrappers.py:390-408
 *   rc_trajectory_slab .......... the per-step transition Collect.step records
 *                                 dreamer/wrappers.py:213-219 (+ dreamer/callbacks.py:41-53)
 *   rc_gather_trajectory ........ the concatenation of those records over all envs, which in the reference is
 *                                 one process appending to one episode list (dreamer/wrappers.py:220-226,
 *                                 dreamer/tools.py:235-264 reads them back); here the envs live on several GPUs
 *                                 and the concat is an RCCL all-gather
 *
 * Conventions
 *   - every function returns RC_OK (0) or a negative rc_status; the message of the last
 *     failure on the calling thread is rc_last_error().  No exception crosses the ABI.
 *   - one rc_env = one GPU + one HIP stream.  Calls on one handle must be serialised by the
 *     caller (the reference callers are single threaded); different handles are independent and
 *     may be driven from different host threads: every entry point selects the handle's device
 *     itself (hipSetDevice), whatever the calling thread's current device is.
 *   - the library owns all device buffers for the handle's lifetime unless the caller passes
 *     `external_arena`; rc_get() returns borrowed device pointers.
 *   - all work is stream-ordered on the handle's stream; rc_sync() waits for it.
 *   - car index c = env * cars_per_env + agent.  Arrays are SoA, one section per field.
 */
#ifndef RACECAR_HIP_H
#define RACECAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 3      /* 3 (round 6): RC_OBS_LIDAR_OCCUPANCY_REFERENCE + rc_set_source_frame; starts never touch a wall on narrow maps
                               * 2 (round 4): rc_build_id, reset laws of SURVEY H6, outbound ordering of the peer-copy gather */
#define RC_N_BEAMS 1080
#define RC_PATCH 64
#define RC_MAX_CARS 4

typedef struct rc_env rc_env;

typedef enum rc_status {
    RC_OK = 0,
    RC_ERR_INVALID = -1,      /* bad argument / call order            */
    RC_ERR_HIP = -2,          /* a HIP runtime call failed            */
    RC_ERR_NO_TRACK = -3,     /* rc_load_track has not been called    */
    RC_ERR_NEEDS_RESET = -4,  /* step before reset ("Must reset environment.", wrappers.py:148) */
    RC_ERR_NOMEM = -5,
    RC_ERR_COMM = -6          /* RCCL could not be loaded or a collective call failed */
} rc_status;

enum { RC_TASK_MAX_PROGRESS = 0, RC_TASK_MAX_SPEED = 1,             /* scenario yml task_name; tasks.py:4-22 */
       RC_TASK_N_STEP_PROGRESS = 2 };  /* secondary agents, baselines/scenarios/max_progress/columbia.yml:17-18: reward =
                                          100 x total progress gained over the last n_steps sub-steps; never done */
#define RC_NSTEP_MAX 16
enum { RC_RESET_GRID = 0, RC_RESET_RANDOM = 1, RC_RESET_RANDOM_BALL = 2 };  /* dream.py:105-108,120 */
enum { RC_OBS_LIDAR = 0, RC_OBS_LIDAR_OCCUPANCY = 1,                  /* dream.py obs_type */
       RC_OBS_LIDAR_OCCUPANCY_REFERENCE = 2 };   /* lidar_occupancy computed EXACTLY as the reference's OccupancyMapObs.step does
                                                  * (dreamer/wrappers.py:396-406: to_pixel, 220 x 220 crop, cubic-spline rotation,
                                                  * centre crop, antialiased bicubic resize) instead of by the one-tap sampler of
                                                  * RC_OBS_LIDAR_OCCUPANCY: bit-identical to the reference's patches, ~500 x the render's cost (0.5 us per car);
                                                  * needs rc_set_source_frame */
/* what RC_F_LIDAR holds: metres, or the caller-side scaling fused into the scan's store */
enum { RC_LIDAR_METRES = 0,
       RC_LIDAR_DREAMER = 1,      /* range / 15 - 0.5              tools.preprocess, dreamer/tools.py:274          */
       RC_LIDAR_UNIT = 2 };       /* (range - 0) * (1 / (15 - 0))  NormalizeObservations, single_agent.py:92-99   */

/* Output / state fields, for rc_get() and rc_copy_out().  n = num_envs * cars_per_env. */
typedef enum rc_field {
    /* --- trajectory record, contiguous in this order (rc_trajectory_slab) --- */
    RC_F_LIDAR = 0,          /* float32 [n, 1080]  ranges [m], beam 0 at +135 deg, clockwise  */
    RC_F_POSE = 1,           /* float32 [n, 6]     x, y, 0, 0, 0, yaw                          */
    RC_F_VELOCITY = 2,       /* float32 [n, 6]     v, 0, 0, 0, 0, yaw rate                     */
    RC_F_SPEED = 3,          /* float32 [n]        |v|   (RaceCarWrapper.step, wrappers.py:66) */
    RC_F_ACTION = 4,         /* float32 [n, 2]     the action passed to rc_step                */
    RC_F_REWARD = 5,         /* float32 [n]        summed over the repeated sub-steps          */
    RC_F_DISCOUNT = 6,       /* float32 [n]        1 - done               (wrappers.py:217)    */
    RC_F_PROGRESS_TOTAL = 7, /* float32 [n]        lap + progress - 1     (wrappers.py:218)    */
    RC_F_TIME = 8,           /* float32 [n]        simulated seconds      (wrappers.py:219)    */
    RC_F_OCCUPANCY = 9,      /* uint8   [n, 64, 64] lidar_occupancy, 1 = drivable (only if enabled) */
    /* --- info / flags --- */
    RC_F_PROGRESS = 10,      /* float32 [n]  norm. distance from start in [0, 1]               */
    RC_F_LAP = 11,           /* int32   [n]  first lap is 1                                    */
    RC_F_CHECKPOINT = 12,    /* int32   [n]                                                    */
    RC_F_DONE = 13,          /* uint8   [n]                                                    */
    RC_F_TRUNCATED = 14,     /* uint8   [n]  done because of time_limit_steps                  */
    RC_F_WALL_COLLISION = 15,     /* uint8 [n]                                                 */
    RC_F_OPPONENT_COLLISION = 16, /* uint8 [n]                                                 */
    RC_F_WRONG_WAY = 17,     /* uint8   [n]                                                    */
    RC_F_FRESH = 18,         /* uint8   [n]  1 if the observation is the first of a new episode */
    RC_F_ACCELERATION = 19,  /* float32 [n]  longitudinal acceleration                          */
    RC_F_STEERING_ANGLE = 20,/* float32 [n]  front wheel angle [rad]                            */
    RC_F_ACTION_IN = 21,     /* float32 [n, 2] device-side action input buffer (writable)       */
    RC_F_COUNT = 22
} rc_field;

/* Kernels, for rc_kernel_time(). */
enum { RC_K_DYNAMICS = 0, RC_K_RAYCAST = 1, RC_K_PATCH = 2, RC_K_RESET = 3, RC_K_ACTIONS = 4, RC_K_FTG = 5, RC_K_POLICY = 6, RC_K_COUNT = 7 };

typedef struct rc_config {
    uint32_t struct_size;          /* = sizeof(rc_config), for ABI evolution                   */
    int32_t  device;               /* HIP device ordinal                                       */
    int32_t  num_envs;             /* envs held by this handle (this GPU's shard)              */
    int32_t  cars_per_env;         /* 1..RC_MAX_CARS                                           */
    int64_t  first_env;            /* global index of env 0: RNG streams are keyed by the global
                                      env id, so results do not depend on the sharding         */
    int32_t  obs_type;             /* RC_OBS_LIDAR | RC_OBS_LIDAR_OCCUPANCY                    */
    int32_t  task;                 /* RC_TASK_*                                                */
    int32_t  laps;                 /* scenario params, dreamer/scenarios/max_progress/columbia.yml:10 */
    float    time_limit;           /*   seconds of simulated time                              */
    int32_t  terminate_on_collision;
    float    collision_reward;
    int32_t  remap_actions;        /* 1: a' = (a + 1) / 2 * (high - low) + low (wrappers.py:128-130) */
    float    action_low[2];        /*   (motor, steering), dream.py:138                        */
    float    action_high[2];
    int32_t  time_limit_steps;     /* TimeLimit duration in rc_step calls; 0 = off (wrappers.py:137-158) */
    int32_t  auto_reset;           /* 1: finished envs are reset inside rc_step (batched rollouts) */
    int32_t  lidar_transform;      /* RC_LIDAR_*: scaling applied when the scan is stored                  */
    void    *external_arena;       /* optional caller-owned device memory for the output arena */
    size_t   external_arena_bytes; /*   must be >= rc_arena_bytes(cfg)                         */
    void    *stream;               /* optional hipStream_t to run on; NULL = library creates one */
    int32_t  car_task[RC_MAX_CARS];/* task of car slot a (agents A, B, C, D of a scenario yml); -1 = `task`          */
    int32_t  n_steps;              /* RC_TASK_N_STEP_PROGRESS window in sub-steps, 1..RC_NSTEP_MAX (yml n_steps: 10) */
    /* Several handles filling ONE arena - one handle per track, so that a batch can mix tracks by blocks of envs (SURVEY.md
     * 8e "per-env track"; BASELINE configs[4] on one GPU): the arena (external_arena) is laid out for arena_total_cars cars
     * and this handle's cars are cars arena_first_car ... of it; every output section then holds the cars of all handles in
     * order.  0 / 0 = the arena is this handle's alone.  rc_trajectory_slab, the compact record and the gathers belong to the
     * arena's owner then, not to a slice handle.  Give each handle first_env = the global index of its first env. */
    int32_t  arena_total_cars;
    int32_t  arena_first_car;
} rc_config;

/* Fill `cfg` with the defaults of the reference's max_progress scenario. */
void rc_default_config(rc_config *cfg);

/* Bytes of device memory the output arena needs for this configuration (for arena_total_cars cars if that is set). */
size_t rc_arena_bytes(const rc_config *cfg);
/* Where a field's section starts in that arena and how many bytes a car takes in it (0 if the field is not enabled):
 * car c's data at section_offset + c * bytes_per_car. */
int rc_field_layout(const rc_config *cfg, int32_t field, size_t *section_offset, size_t *bytes_per_car);

int rc_create(const rc_config *cfg, rc_env **out);
void rc_destroy(rc_env *env);

/*
 * Upload one compiled track (host pointers).  Bitmaps are uint32 [h][pitch], bit i of word j =
 * cell ix = 32*j + i, row iy = 0 is the southern-most.  progress is float32 [h][w]
 * (norm_distance_from_start, generate-costmap.py:220-222; < 0 outside the drivable area),
 * centerline float32 [n][4] = x, y, heading, progress (spawn table for rc_reset).
 */
int rc_load_track(rc_env *env, const uint32_t *occ_words, const uint32_t *drivable_words,
                  const float *progress, int32_t h, int32_t w, int32_t pitch,
                  float resolution, float origin_x, float origin_y,
                  const float *centerline, int32_t n_centerline);

/*
 * Where the track's grid lies in the source image it was cropped from - what the reference's GridMap.to_pixel indexes
 * (dreamer/wrappers.py:396: row = int(H - (y - oy) / res), col = int((x - ox) / res), north-up, the whole image).  Needed by
 * RC_OBS_LIDAR_OCCUPANCY_REFERENCE only, before the first reset: full_height = H; a north-up pixel (R, C) of the image is cell
 * (gx, gy) = (C - col0, row_top - R) of the grid rc_load_track was given; (origin_x, origin_y) = world position of the image's
 * lower left corner; resolution in metres per cell - all three as binary64, as the reference computes with them.
 */
int rc_set_source_frame(rc_env *env, int32_t full_height, int32_t row_top, int32_t col0, double origin_x, double origin_y,
                        double resolution);

/* Reset the envs selected by the host mask (uint8 [num_envs], NULL = all) and produce their
 * first observation. */
int rc_reset(rc_env *env, const uint8_t *mask_or_null, int32_t mode, uint64_t seed);

/* One agent step = up to `repeat` simulator sub-steps of dt = 0.01 s, then the observation.
 * `actions_dev` is device memory float32 [n, 2] = (motor, steering); NULL = use the buffer
 * behind RC_F_ACTION_IN (e.g. after rc_fill_random_actions).  motor >= 0 accelerates, < 0 brakes; a POSITIVE steering command
 * turns RIGHT - towards higher beam indices (beam 0 is at +135 deg on the left) - and +-1 is a front-wheel angle of 0.19 rad:
 * the convention under which the reference's own trained agents (ros_agent/checkpoints) drive (tests/test_golden_policy.py). */
int rc_step(rc_env *env, const float *actions_dev, int32_t repeat);
/* Same, actions in host memory (copied with the stream). */
int rc_step_host(rc_env *env, const float *actions_host, int32_t repeat);

/* Teleport: overwrite every car's pose from host memory, float32 [n, 3] = x, y, yaw (|yaw| <= pi), keep the
 * rest of the state, and recompute the observation (LiDAR, patch).  The analogue of setting the base pose of
 * the vehicle body in the reference's simulator; used by evaluation tooling and by the raycast parity tests. */
int rc_set_pose(rc_env *env, const float *xyyaw_host);

/* Fill RC_F_ACTION_IN with U(-1,1)^2 from Philox4x32-10 keyed by (seed, step, global car id). */
int rc_fill_random_actions(rc_env *env, uint64_t seed, uint32_t step);
/* rc_fill_random_actions(seed, step) followed by rc_step(NULL, repeat) as ONE pass: the dynamics kernel draws the
 * same actions itself (and leaves them in RC_F_ACTION_IN).  The step of a synthetic random-action rollout - the
 * reference's default prefill policy is random actions too (dreamer/dream.py:207-210) - without a
 * launch of its own for the action generator.  Results are identical to the two-call form. */
int rc_step_random(rc_env *env, uint64_t seed, uint32_t step, int32_t repeat);

/* rc_step / rc_step_random of SEVERAL handles as one launch per kernel - the handles of a batch that mixes tracks (one handle
 * per track, each filling its block of cars of ONE arena: rc_config.arena_total_cars / arena_first_car; SURVEY.md 8e "per-env
 * track_id selecting a device-resident grid", BASELINE configs[4]'s track mix).  Every wave of the launch works from the
 * parameters of the block it lies in, so the chip sees one dynamics and one scan kernel over all cars instead of one small pair
 * per track.  The handles share a device, a stream and cars_per_env (at most 8 of them); `actions_dev` is float32 [total cars, 2]
 * in arena order, NULL = every handle's RC_F_ACTION_IN.  Results are those of stepping the handles one by one. */
int rc_step_group(rc_env **envs, int32_t n, const float *actions_dev, int32_t repeat);
int rc_step_random_group(rc_env **envs, int32_t n, uint64_t seed, uint32_t step, int32_t repeat);

/* ---- Domain randomization (per episode), both features opt-in and off by default; with both off every output is what it is
 * without them (the production kernels run).  Each handle has its own settings; rc_step_group honours every handle's.
 *
 * Vehicle parameters: five binary32 values per car, columns of a float32 [n_cars][5] array in this order (nominal values =
 * the spec's constants, bit for bit):
 *   0 wheel_max  [rad]              front-wheel angle at full steering command     0.19   (steering gain = -wheel_max)
 *   1 accel_max  [m/s^2]            longitudinal acceleration at full motor        4.0
 *   2 drag       [1/s]              velocity-proportional deceleration             0.8
 *   3 max_vel    [m/s]              the velocity clamp                             5.0
 *   4 steer_step [rad per sub-step] the steering slew per dt = 0.01 s              0.032
 * The integrator does the same operations in the same order with the car's value as the operand.  The agent-side kernels
 * (rc_follow_the_gap, rc_follow_the_gap_reference) keep mapping a wheel angle to a command with the NOMINAL 0.19 rad: an
 * agent does not know its car.  The parameters are state, not record: rc_arena_bytes, the trajectory slab and the compact
 * slab do not change.
 *
 * rc_set_vehicle_randomization: random mode.  At every reset of an env (rc_reset and the auto-reset inside rc_step) each of
 * its cars draws value_i = lo[i] + u * (hi[i] - lo[i]), u = (w >> 8) * 2^-24, one binary32 rounding per operator (lo == hi
 * gives lo exactly).  Word j = 5 a + i (car slot a, parameter i) is word j % 4 (x, y, z, w) of Philox4x32-10 keyed by `seed`
 * with counter (global env id, episode value the spawn draw of that reset uses, j / 4, 2) - the spawn uses counter word 3 = 0
 * and the random actions their own counters, so starts and actions do not change, and sharding does not change the draw.
 * Takes effect at each env's next reset.  lo or hi NULL = off (every car back to the nominal values).
 * rc_set_vehicle_params: fixed mode.  Copies float32 [n_cars][5] from DEVICE memory (stream-ordered); the values persist
 * across resets and nothing is drawn.  NULL = off.
 * rc_vehicle_params: the handle's device array of the current values, float32 [n_cars][5] (*bytes = n_cars * 20).
 *
 * LiDAR noise (obs lidar only; the occupancy renders do not change): for every beam of every car, after the inter-car minimum
 * and before the lidar_transform scaling,
 *     if r < 15: r = clamp(r + n, 0, 15)       n = (k0 + k1 + k2 + k3 - 8190) * s,  s = fl(sigma * 4.2286398820579052e-4f)
 *     if d < D:  r = 15  (no return)           D = floor(p_drop * 65536 + 0.5)
 * k0..k3 are bits 0-11 and 12-23 of two words w0, w1, d = (w0 >> 24) << 8 | (w1 >> 24): Irwin-Hall(4) of 12-bit uniforms,
 * standardised (zero mean, unit variance: 4.2286398820579052e-4 = sqrt(3 / (4096^2 - 1)) in binary32), z bounded by
 * +- 3.46 sigma; dropout probability D / 65536.  The words come from lowbias32 (two multiply / xor-shift rounds:
 * x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *     key = h(seed_lo ^ h(global car id ^ h(episode ^ h(sub-steps ^ seed_hi))))   (the env's counters as they stand when
 *                                                                                   the scan runs)
 *     w_j = h(key + (2 * beam + j) * 0x9E3779B9), j = 0, 1                        (all arithmetic mod 2^32)
 * so the noise does not depend on which wave or round computes a beam, nor on the sharding.  The uint16 compact copy
 * quantises the noisy value.  sigma = p_drop = 0 = off.  Runs in its own scan instantiations (rc_scan_kernel_name:
 * "rc_raycast_car_noise_kernel<...>"); a lab variant, the bounded validation build and the instrumented build refuse it. */
int rc_set_vehicle_randomization(rc_env *env, const float *lo, const float *hi, uint64_t seed);
int rc_set_vehicle_params(rc_env *env, const float *params_dev);
int rc_vehicle_params(rc_env *env, void **dev_ptr, size_t *bytes);
int rc_set_lidar_noise(rc_env *env, float sigma, float p_drop, uint64_t seed);

/* ---- Track set: a new track at every reset (the reference's ChangingTrackSingleAgentRaceEnv, per env, on the device) --------
 * A handle may carry a track set: T tracks, 1 <= T <= 8 (RC_GROUP_MAX).  Each env has a current track track[e], an int32 in [0, T).
 *   Shared track: all cars of an env are on the env's track.  Car-car collision is unchanged.
 *   Which resets switch: every reset of an env draws its next track BEFORE the spawn draw, then spawns on that track by the
 *   unchanged reset law (grid / random / random_ball, spawn_safe of that track).  This covers rc_reset with or without a mask and
 *   the auto-reset inside rc_step.  One exception: an env's first reset after the track set is installed keeps its initial
 *   assignment.  This is per env, so a masked rc_reset starts only the envs it resets (_ChangingTrack.reset's _started flag).
 *   Orders:
 *     RC_TRACK_ORDER_SEQUENTIAL  track = (track + 1) mod T.
 *     RC_TRACK_ORDER_RANDOM      r = word 0 (x) of Philox4x32-10 keyed by the set's own `seed`, counter (global env id, the episode
 *                                value that reset's spawn draw uses, 0, 3) - counter word 3 = 3 is free: the spawn and the random
 *                                actions use 0, vehicle randomization 2, window sampling 0x57494e44.  track = (r * T) >> 32 (the
 *                                law of the spawn bin).  With weights w_0..w_{T-1} (finite, > 0): track = the number of k in
 *                                [1, T) with c_k <= r, c_k = min(floor(2^32 * S_k / S + 0.5), 2^32 - 1), S_k = w_0 + ... + w_{k-1}
 *                                and S = w_0 + ... + w_{T-1} summed in binary64 from the binary32 weights (rounded half up once).
 *     RC_TRACK_ORDER_MANUAL      track = next[e], a device int32 array the caller writes (rc_set_next_track).  It persists and is
 *                                read at each reset; a value outside [0, T) keeps the current track.
 *   Sharding: the draw depends only on the global env id and the episode, so a shard (first_env) sees the tracks of the full job.
 *   Outputs: after a step track[e] names the track of the observation in the arena; after an auto-reset that is the new episode's
 *   track, and the first patch stays all zeros as before.
 *   Layout: the track ids are state, not record: rc_arena_bytes, the trajectory slab, the compact slab and RC_ABI_VERSION do not
 *   change.
 *   Vehicle randomization and LiDAR noise compose with a track set.
 *   Refused (RC_ERR_INVALID): obs_type RC_OBS_LIDAR_OCCUPANCY_REFERENCE (its exact render holds per-handle scratch from
 *   rc_set_source_frame); a track-set handle in rc_step_group / rc_step_random_group; a lab scan variant, the bounded validation
 *   build and the instrumented scan (at the next observation, as the noise scan); rc_set_pose.
 *
 * rc_set_track_set: tracks[0..n) are handles that went through rc_load_track on the same device (the owner itself may be one of
 * them; a small handle, 1 env, is enough: only its track tables are used).  They must outlive the owner, or the next
 * rc_set_track_set.  order: RC_TRACK_ORDER_*.  weights_or_null: T floats (order random only).  initial_dev_or_null: int32
 * [num_envs] in DEVICE memory, each in [0, n) (copied and checked at the call); NULL = contiguous blocks of near-equal size, the
 * first num_envs % n tracks one env longer (MixedTrackEnv's split).  The next-track array of manual order starts as the initial
 * assignment.  Takes effect at each env's next reset (the first keeps `initial`).  n = 0 turns the feature off: the production
 * kernels run again and rc_scan_kernel_name reports their name.
 * rc_set_next_track: copies int32 [num_envs] from DEVICE memory (stream-ordered) into the next-track array of manual order.
 * rc_track_ids: the handle's device array of the current tracks, int32 [num_envs] (*bytes = num_envs * 4); valid once a track
 * set has been installed.
 * Kernels: rc_dynamics_ts_kernel / rc_reset_ts_kernel (per-lane track tables), rc_ts_count / start / place_kernel (the cars track-major every
 * observation), rc_raycast_ts_kernel (rc_scan_kernel_name: "rc_raycast_ts_kernel<A, split, noise>"), rc_patch_ts_kernel. */
enum { RC_TRACK_ORDER_SEQUENTIAL = 0, RC_TRACK_ORDER_RANDOM = 1, RC_TRACK_ORDER_MANUAL = 2 };
int rc_set_track_set(rc_env *env, rc_env *const *tracks, int32_t n, int32_t order, const float *weights_or_null,
                     const int32_t *initial_dev_or_null, uint64_t seed);
int rc_set_next_track(rc_env *env, const int32_t *next_dev);
int rc_track_ids(rc_env *env, void **dev_ptr, size_t *bytes);

/* Batched follow-the-gap agent on the device (the prefill / baseline agent of dreamer/dream.py:211-216, whose
 * host form is agents.gap_follower.GapFollower): from the current LiDAR scan of every car, clip to 6 m,
 * 5-beam smoothing over the forward 202.5 deg, safety bubble of +-60 beams around the closest return, point the wheels at
 * the centre of the widest run of beams whose smoothed range exceeds 2 m (full lock beyond 0.19 rad).  Writes (motor, steering) into RC_F_ACTION_IN: steering in [-1, 1],
 * motor = motor_corner if |steering| > 0.35 else motor_straight (values in the caller's action convention). */
int rc_follow_the_gap(rc_env *env, float motor_straight, float motor_corner);

/* The REFERENCE's follow-the-gap law on the device (ros_agent/agents/follow_the_gap/src/agent.py:128-193: forward arc
 * of +-90 deg clipped at the look-ahead distance, disparities found with 10-degree median / maximum filters and extended
 * by the vehicle's half-width, heading = mean angle of the beams at or above the 83.3rd percentile; :200-234: steering =
 * 1.4 heading - 0.1 d(heading)/dt clipped to +-24 deg, speed 6 m/s less up to 30 % with the steering angle, at most 4/5
 * of the free distance below 5 m, at least 1.5 m/s).  Writes (motor, steering) into RC_F_ACTION_IN - the node's speed over
 * the car's top speed, and the command that puts the front wheels at the node's steering angle (positive command = right; full
 * lock beyond the car's 0.19 rad), in the caller's action convention (the remap of
 * rc_config is inverted when it is on).  dt = seconds per agent step (the derivative term; none on an episode's first
 * command).  detail_dev: optional device float32 [n, 4] = heading [rad], free distance [m], steering angle [rad], speed
 * [m/s].  The generic bubble / widest-gap agent above stays available as rc_follow_the_gap. */
int rc_follow_the_gap_reference(rc_env *env, float dt, float *detail_dev);

/* The reference's trained Dreamer agent on the device, deterministic mode (ros_agent/models/dreamer/racing_dreamer.py:61-80
 * `action`: obs_step from the previous latent and the previous RAW action, feature = [stoch, deter], actor mode;
 * models.py:61-87 RSSM.obs_step / img_step, :339-364 ActionDecoder 'tanh_normal' and actor_version "normalized") - the posterior
 * MEAN instead of a sample and tanh(mean) instead of the best of 100 draws, in the binary32 arithmetic of DESIGN.md §2 item 12
 * (tests/policy_spec.c is its CPU restatement; the device equals it bit for bit).  rc_policy_set_sampling switches to the
 * reference's own sampled modes; rc_policy_imagine (below) runs the prior and the reward head, rc_policy_decode
 * (below it) the observation decoder.
 *
 * rc_policy_weights: host pointers and shapes of the checkpoint's arrays in `tf.Module.variables` order (rssm.pkl: 13 arrays,
 * actor.pkl: 10, or 14 with the batch normalisation's four).  One-dimensional arrays have rows = 1. */
typedef struct rc_policy_array { const float *data; int32_t rows, cols; } rc_policy_array;
typedef struct rc_policy_weights {
    uint32_t struct_size;          /* = sizeof(rc_policy_weights) */
    rc_policy_array gru_kernel, gru_recurrent, gru_bias;      /* [200, 600] x 2, [2, 600]: gates z, r, candidate; reset_after */
    rc_policy_array img1_w, img1_b;                            /* [32, 200], [200]    input [stoch 30, previous action 2]      */
    rc_policy_array img2_w, img2_b, img3_w, img3_b;            /* the prior's layers: read by rc_policy_imagine only (data may be
                                                                  NULL: the agent works, imagination is refused; checked when
                                                                  given: [200, 200], [200], [200, 60], [60])                   */
    rc_policy_array obs1_w, obs1_b, obs2_w, obs2_b;            /* [1280, 200], [200], [200, 60], [60]   input [deter, scan]    */
    rc_policy_array h0_w, h0_b, h1_w, h1_b, h2_w, h2_b, h3_w, h3_b;   /* [230, 400], [400], 3 x ([400, 400], [400])            */
    rc_policy_array hout_w, hout_b;                            /* [400, 4], [4]                                                */
    rc_policy_array hnorm_mean, hnorm_var, hnorm_gamma, hnorm_beta;   /* [4] each, or all four data = NULL: the plain actor     */
} rc_policy_weights;
/* rc_policy_load (racing_dreamer.py:9-41, the constructor's load of rssm.pkl / actor.pkl): checks the shapes (RC_ERR_INVALID
 * names the first that is wrong - before anything else, so a caller can validate a checkpoint without a handle), copies the
 * weights to the handle's device and allocates the agent's state, zeroed: float32 [n_cars, 232] = stoch 30 | deter 200 | raw
 * previous action 2.  A second load replaces the weights and zeroes the state.  rc_policy_unload frees both. */
int rc_policy_load(rc_env *env, const rc_policy_weights *w);
int rc_policy_unload(rc_env *env);
/* rc_policy_act (racing_dreamer.py:61-80): one agent step for every car whose slot (car index within its env) is in slot_mask
 * (bit a = slot a).  Reads RC_F_LIDAR in place - in metres: refused under another lidar_transform - and RC_F_FRESH: a car whose
 * observation opens an episode starts from a zero latent and a zero previous action (racing_dreamer.py:66-70).  Writes the
 * car's state and its command into RC_F_ACTION_IN in the caller's action convention: the raw action in [-1, 1]^2 when
 * rc_config.remap_actions is on (the env applies ReduceActionSpace), else postprocess_action's image of it
 * (racing_dreamer.py:53-59) in [action_low, action_high].  The state always keeps the raw action.  Cars outside the mask keep
 * their RC_F_ACTION_IN and state rows.  RC_ERR_INVALID: no policy loaded, empty mask, bits beyond cars_per_env, scan not in
 * metres.  Kernel: rc_policy_kernel (RC_K_POLICY). */
int rc_policy_act(rc_env *env, uint32_t slot_mask);
/* The agent's state (models.py:61-87: the RSSM's stoch and deter; racing_dreamer.py:76: the previous action), zero-copy:
 * device float32 [n_cars, 232], readable and writable between calls. */
int rc_policy_state(rc_env *env, void **dev_ptr, size_t *bytes);
/* The sampled modes: the agent as the reference itself runs it (tests/policy_sample_spec.c is the CPU
 * restatement, the device equals it bit for bit).
 *   RC_POLICY_MODE_MEAN     posterior mean, tanh(mean): the deterministic mode above, the default.
 *   RC_POLICY_MODE_DEPLOY   the deployed / evaluation agent (ros_agent/models/dreamer/racing_dreamer.py:61-80, dreamer/models.py:66-81
 *                           with training=False, run_evaluation.py): the posterior is SAMPLED (RSSM.obs_step: stoch =
 *                           Normal(mean, softplus(raw) + 0.1).sample()), the action is SampleDist.mode() - of
 *                           RC_POLICY_MODE_SAMPLES tanh-normal draws the one with the highest log-probability
 *                           (dreamer/tools.py:301-321), chosen per car - clipped to +-1.  expl_amount 0 = the reference's eval_noise off.
 *   RC_POLICY_MODE_EXPLORE  the training-time collector (dreamer/models.py:75-79, 189-202, dream.py:96-99): the posterior sampled,
 *                           ONE action draw actor(feat).sample(), then additive_gaussian exploration clip(Normal(action,
 *                           expl_amount).sample(), -1, 1); the clipped action is the command and the next step's previous action.
 * The draws are Philox4x32-10 keyed by `seed` and counted by (global env id, the env's episode counter, its agent step within the
 * episode, slot and index): a function of those only - not of the shard (rc_config.first_env), the slot mask or the call history.
 * Two rc_policy_act calls without a step in between draw the same numbers. */
#define RC_POLICY_MODE_MEAN 0
#define RC_POLICY_MODE_DEPLOY 1
#define RC_POLICY_MODE_EXPLORE 2
#define RC_POLICY_MODE_SAMPLES 100
typedef struct rc_policy_sampling {
    uint32_t struct_size;          /* = sizeof(rc_policy_sampling) */
    int32_t mode;                  /* RC_POLICY_MODE_* */
    uint64_t seed;
    float expl_amount;             /* standard deviation of the additive exploration noise (dream.py:96-99: 0.3 while collecting), >= 0 */
} rc_policy_sampling;
/* rc_policy_set_sampling: the mode of the rc_policy_act calls that follow, until it is changed or the policy is unloaded;
 * rc_policy_load resets it to RC_POLICY_MODE_MEAN.  s = NULL: RC_POLICY_MODE_MEAN.  RC_ERR_INVALID: wrong struct_size, unknown
 * mode, expl_amount negative or not finite, no policy loaded.  Kernel of the sampled modes: rc_policy_sampled_kernel, timed
 * under RC_K_POLICY.  rc_policy_get_sampling: what is installed. */
int rc_policy_set_sampling(rc_env *env, const rc_policy_sampling *s);
int rc_policy_get_sampling(rc_env *env, rc_policy_sampling *out);

/* Imagination: the world model rolled ahead from every car's stored latent, and its reward head (DESIGN.md §2 item 15;
 * tests/policy_imagine_spec.c is the CPU restatement, the device equals it bit for bit).  For t = 0 .. horizon - 1: the action is
 * the caller's actions_in[car, t] (open loop: ros_agent/models/dreamer/models.py:44-52 RSSM.imagine; raw, clamped to [-1, 1]) or
 * the actor's on [stoch, deter] (closed loop: dreamer/models.py:213-224 _imagine_ahead); then the prior step img_step
 * (models.py:72-84); feature[t] = [stoch', deter'], reward[t] = the reward head on it (models.py:301-318 DenseDecoder).
 *   RC_POLICY_IMAGINE_MEAN     action tanh(mu), stoch' = the prior's mean: deterministic.
 *   RC_POLICY_IMAGINE_SAMPLE   one tanh-normal action draw (the reference's actor(feat).sample(); no best of 100, no exploration
 *                              noise) and stoch' ~ Normal(mean, softplus(raw) + 0.1), Philox4x32-10 keyed by `seed` and counted by
 *                              (global env id, episode, agent step, slot, t, index): not by the shard, the mask or the call history.
 * The "normalized" actor uses its moving statistics, as rc_policy_act does.  A pure function of the latent as rc_policy_act last
 * left it (RC_F_FRESH is not looked at): the agent's state, RC_F_ACTION_IN, the arena and every counter stay as they are.
 *
 * rc_policy_heads: the reward head's arrays, host pointers as in rc_policy_weights.  rc_policy_load_heads checks the shapes first
 * (RC_ERR_INVALID names the first that is wrong), needs a loaded policy and copies the arrays; h = NULL drops the head, and so do
 * rc_policy_load and rc_policy_unload. */
typedef struct rc_policy_heads {
    uint32_t struct_size;          /* = sizeof(rc_policy_heads) */
    rc_policy_array reward_h0_w, reward_h0_b;                  /* [230, 400], [400]   input [stoch, deter]                     */
    rc_policy_array reward_h1_w, reward_h1_b;                  /* [400, 400], [400]                                            */
    rc_policy_array reward_hout_w, reward_hout_b;              /* [400, 1], [1]                                                */
} rc_policy_heads;
int rc_policy_load_heads(rc_env *env, const rc_policy_heads *h);
#define RC_POLICY_IMAGINE_MEAN 0
#define RC_POLICY_IMAGINE_SAMPLE 1
#define RC_POLICY_IMAGINE_MAX_HORIZON 64
#define RC_POLICY_FEATURE 230      /* stoch 30 | deter 200 */
typedef struct rc_policy_imagine_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_imagine_args) */
    int32_t horizon;               /* H in [1, RC_POLICY_IMAGINE_MAX_HORIZON]; the reference's is 15 */
    int32_t mode;                  /* RC_POLICY_IMAGINE_* */
    uint32_t slot_mask;            /* bit a = slot a, as rc_policy_act's */
    uint64_t seed;
    const float *actions_in;       /* device float32 [n_cars, H, 2], or NULL: the actor's own actions */
    float *reward;                 /* device float32 [n_cars, H], or NULL */
    float *actions;                /* device float32 [n_cars, H, 2], or NULL: the actions taken (open loop: the clamped input) */
    float *features;               /* device float32 [n_cars, H, 230], or NULL */
    float *reward_start;           /* device float32 [n_cars], or NULL: the head on the starting feature */
} rc_policy_imagine_args;
/* rc_policy_imagine: one launch for the whole horizon, on the handle's stream.  Rows are indexed by car; rows of cars outside
 * the mask are not touched.  RC_ERR_INVALID: wrong struct_size, no policy loaded, the policy loaded without img2 / img3,
 * horizon outside [1, 64], unknown mode, empty mask or bits beyond cars_per_env, no output asked for, reward or reward_start
 * asked for without a loaded head.  Kernels: rc_policy_imagine_kernel, rc_policy_imagine_sampled_kernel, timed under RC_K_POLICY. */
int rc_policy_imagine(rc_env *env, const rc_policy_imagine_args *args);

/* Planning in the latent: K candidate action sequences per start latent, carried through the world model and scored by its reward
 * head (tests/policy_dream_spec.c is the CPU restatement, the device equals it bit for bit) - the dream's
 * counterpart of rc_look_ahead, what PlaNet-style random shooting or the cross-entropy method ask of a world model.  Rows are pairs
 * (start s, candidate k), k in [0, candidates); all K rows of a start begin from the same latent:
 *   state_in = NULL   the live latents of rc_policy_state: one start per car whose slot is in slot_mask, as rc_policy_imagine; the
 *                     arrays are indexed by car ([n_cars, K, ...]), rows of cars outside the mask are not touched; RC_F_FRESH is
 *                     not looked at.  The start id is the global car id (first_env + env) * cars_per_env + slot.
 *   state_in given    device float32 [starts, 232] in rc_policy_state's layout (the last two columns are not read; rc_policy_observe's
 *                     state_out fits as it is: observe a replay window, then plan from its end).  Nothing to do with the env's cars:
 *                     slot_mask must be 0.  The start id is row_offset + s (64 bits).
 * For t = 0 .. horizon - 1 a row does what open-loop rc_policy_imagine does: a = clamp(actions_in[s, k, t], -1, 1); the prior step
 * img_step (ros_agent/models/dreamer/models.py:44-52 RSSM.imagine: img1, GRU, img2, img3); the reward head on the new feature
 * (dreamer/models.py:301-318 DenseDecoder).  The actor is never run.  Modes are rc_policy_imagine's: RC_POLICY_IMAGINE_MEAN, and
 * RC_POLICY_IMAGINE_SAMPLE: stoch' ~ Normal(mean, softplus(raw) + 0.1), Philox4x32-10 keyed by `seed` and counted by (start id,
 * candidate, t, index) under tag 7 (counter word 3, bits 24-31) - not by K, the workgroup, the mask, the shard or the call history;
 * a caller who wants fresh draws at every step changes `seed`.
 * Outputs, each optional, at least one: ret [starts, K] = sum_t discount^t r_t, accumulated in binary32 in step order (acc = 0, w = 1;
 * acc = fmaf(w, r_t, acc); w = w * discount); reward [starts, K, H]; final_feature [starts, K, 230] = the feature after step H - 1
 * (for a caller's own value head: a bootstrap value).  A pure function of its inputs: the agent's state, RC_F_ACTION_IN, the arena,
 * the episode log and every counter stay as they are. */
typedef struct rc_policy_dream_ahead_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_dream_ahead_args) */
    int32_t horizon;               /* H in [1, RC_POLICY_IMAGINE_MAX_HORIZON] */
    int32_t mode;                  /* RC_POLICY_IMAGINE_* */
    int32_t candidates;            /* K >= 1; starts x K < 2^31 */
    uint32_t slot_mask;            /* live latents: bit a = slot a, as rc_policy_act's; with state_in: 0 */
    float discount;                /* in [0, 1]; 1: the plain sum */
    uint64_t seed;
    int64_t starts;                /* with state_in: its rows, >= 1 (live latents: not read) */
    uint64_t row_offset;           /* with state_in: the start id of start 0 (mode SAMPLE) */
    const float *state_in;         /* device float32 [starts, 232], or NULL: the live latents */
    const float *actions_in;       /* device float32 [starts, K, H, 2], raw in [-1, 1] (clamped) */
    float *ret;                    /* device float32 [starts, K], or NULL */
    float *reward;                 /* device float32 [starts, K, H], or NULL */
    float *final_feature;          /* device float32 [starts, K, 230], or NULL */
} rc_policy_dream_ahead_args;
/* rc_policy_dream_ahead: one launch on the handle's stream.  RC_ERR_INVALID: wrong struct_size, no policy loaded, the policy loaded
 * without img2 / img3, ret or reward asked for without a loaded head, horizon outside [1, 64], candidates < 1 or starts x candidates
 * not below 2^31, unknown mode, discount not finite or outside [0, 1], actions_in NULL, no output asked for, state_in together with
 * a non-zero mask or starts < 1, live latents with an empty mask or bits beyond cars_per_env.  Kernels: rc_policy_dream_kernel,
 * rc_policy_dream_sampled_kernel, timed under RC_K_POLICY. */
int rc_policy_dream_ahead(rc_env *env, const rc_policy_dream_ahead_args *args);

/* The dream's backward pass: the gradient of rc_policy_dream_ahead's return with respect to the raw action sequence and to the start
 * latent (tests/policy_dream_grad_spec.c is the CPU restatement, the device equals it bit for bit) - what
 * gradient-based planning in the latent asks of a world model.  Starts, rows, modes, the draws and their keys are
 * rc_policy_dream_ahead's; the forward is its step, and `ret` and `reward` come out byte for byte as it gives them.  The backward
 * differentiates, for t = horizon - 1 .. 0, the reward head (dreamer/models.py:301-318 DenseDecoder) and the prior step
 * (models.py:369-380 RSSM.img_step: img1, the GRU, img2, img3 and, in mode SAMPLE, stoch' = mean + (softplus(raw) + 0.1) n with the
 * step's own normal n held fixed) with respect to their inputs only: no weight gradient.  The clamp of the raw action to [-1, 1]
 * passes the gradient where -1 <= a <= 1 (inclusive, as tf.clip_by_value) and gives exactly +0 elsewhere.
 * Outputs, each optional, at least one: grad_actions [starts, K, H, 2] = d ret / d actions_in; grad_state [starts, K, 230] = d ret /
 * d (stoch | deter) of the start; ret [starts, K]; reward [starts, K, H].  A reward head must be loaded.  The activations of the
 * forward are kept in a scratch the handle owns (2 240 floats per row and step, at most 1 GiB, grown on demand, released with the
 * policy); the rows are cut into chunks of chunk_rows (0: as many as the scratch's limit holds), one launch per chunk - the results
 * do not depend on the chunking.  A pure function of its inputs otherwise, as rc_policy_dream_ahead. */
typedef struct rc_policy_dream_grad_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_dream_grad_args) */
    int32_t horizon;               /* H in [1, RC_POLICY_IMAGINE_MAX_HORIZON] */
    int32_t mode;                  /* RC_POLICY_IMAGINE_* */
    int32_t candidates;            /* K >= 1; starts x K < 2^31 */
    uint32_t slot_mask;            /* live latents: bit a = slot a, as rc_policy_act's; with state_in: 0 */
    float discount;                /* in [0, 1]; 1: the plain sum */
    uint64_t seed;
    int64_t starts;                /* with state_in: its rows, >= 1 (live latents: not read) */
    uint64_t row_offset;           /* with state_in: the start id of start 0 (mode SAMPLE) */
    int64_t chunk_rows;            /* rows per launch, rounded up to a multiple of 32; 0: derived from the scratch's limit */
    const float *state_in;         /* device float32 [starts, 232], or NULL: the live latents */
    const float *actions_in;       /* device float32 [starts, K, H, 2], raw */
    float *grad_actions;           /* device float32 [starts, K, H, 2], or NULL */
    float *grad_state;             /* device float32 [starts, K, 230], or NULL */
    float *ret;                    /* device float32 [starts, K], or NULL */
    float *reward;                 /* device float32 [starts, K, H], or NULL */
} rc_policy_dream_grad_args;
/* rc_policy_dream_grad: one launch per chunk on the handle's stream.  RC_ERR_INVALID: as rc_policy_dream_ahead, and no reward head
 * loaded whatever is asked for, chunk_rows < 0.  Kernels: rc_policy_dream_grad_kernel, rc_policy_dream_grad_sampled_kernel (and, at
 * the first call after the weights were loaded, rc_policy_dream_grad_transpose_kernel), timed under RC_K_POLICY. */
int rc_policy_dream_grad(rc_env *env, const rc_policy_dream_grad_args *args);

/* The critic and the lambda-return: the forward half of the reference's behaviour learning (dreamer/models.py:113-133 in
 * `Dreamer.train`; tests/policy_returns_spec.c is the CPU restatement, the device equals it bit for bit).
 * The rollout is rc_policy_imagine's - closed loop under the actor or open loop under actions_in, in its two modes - and on every
 * imagined feature run the reward head, the value head (value(feat).mode()) and the pcont head (pcont(feat).mean() = sigmoid of
 * the logit), each DenseDecoder (models.py:301-318) and each only when an output needs it.  Then, with r, v, p [H] of a row and
 * p_t = discount where no pcont head is loaded (dreamer/tools.py:396-418 `lambda_return` through `static_scan(reverse=True)`, and
 * models.py:121-125's cumprod), in binary32:
 *   R_{H-1} = v_{H-1};  for t = H - 2 .. 0:  in_t = fmaf(p_t * v_{t+1}, 1 - lambda_, r_t),  R_t = fmaf(p_t * lambda_, R_{t+1}, in_t)
 *   returns[t] = R_t;  weight[0] = 1,  weight[t] = weight[t-1] * p_{t-1}                                          (t < H - 1)
 * Starts:
 *   state_in = NULL   the live latents of rc_policy_state, one per car whose slot is in slot_mask; arrays are indexed by car, rows
 *                     of cars outside the mask are not touched; the draws of RC_POLICY_IMAGINE_SAMPLE are rc_policy_imagine's
 *                     own, so the same seed gives the same dream.
 *   state_in given    device float32 [starts, 232] in rc_policy_state's layout (the last two columns are not read); slot_mask
 *                     must be 0.  The draws are keyed by `seed` and counted by (row_offset + row, t, index) under tag 8 (counter
 *                     word 3, bits 24-31): not by the workgroup, the shard or the call history.
 * horizon = 0 runs the heads on the starting features alone (the *_start outputs): the same entry scores arbitrary features.
 *
 * rc_policy_critic: the two heads' arrays, host pointers as in rc_policy_heads; the pcont head is optional as a whole (all its
 * data pointers NULL).  rc_policy_load_critic checks the shapes first (RC_ERR_INVALID names the first that is wrong), needs a
 * loaded policy and copies the arrays; h = NULL drops both heads, and so do rc_policy_load and rc_policy_unload. */
typedef struct rc_policy_critic {
    uint32_t struct_size;          /* = sizeof(rc_policy_critic) */
    rc_policy_array value_h0_w, value_h0_b;                    /* [230, 400], [400]   input [stoch, deter]                     */
    rc_policy_array value_h1_w, value_h1_b;                    /* [400, 400], [400]                                            */
    rc_policy_array value_h2_w, value_h2_b;                    /* [400, 400], [400]                                            */
    rc_policy_array value_hout_w, value_hout_b;                /* [400, 1], [1]                                                */
    rc_policy_array pcont_h0_w, pcont_h0_b;                    /* the same shapes, or all eight data = NULL: no pcont head     */
    rc_policy_array pcont_h1_w, pcont_h1_b;
    rc_policy_array pcont_h2_w, pcont_h2_b;
    rc_policy_array pcont_hout_w, pcont_hout_b;
} rc_policy_critic;
int rc_policy_load_critic(rc_env *env, const rc_policy_critic *h);
typedef struct rc_policy_returns_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_returns_args) */
    int32_t horizon;               /* H in [0, RC_POLICY_IMAGINE_MAX_HORIZON]; 0: *_start outputs only; returns, weight: H >= 2 */
    int32_t mode;                  /* RC_POLICY_IMAGINE_* */
    uint32_t slot_mask;            /* live latents: bit a = slot a, as rc_policy_act's; with state_in: 0 */
    float lambda_;                 /* in [0, 1]; the reference's disclam is 0.95 */
    float discount;                /* in [0, 1]: the constant pcont when no pcont head is loaded; the reference's is 0.99 */
    uint64_t seed;
    int64_t starts;                /* with state_in: its rows, in [1, 2^31) (live latents: not read) */
    uint64_t row_offset;           /* with state_in: the id of row 0 (mode SAMPLE) */
    const float *state_in;         /* device float32 [starts, 232], or NULL: the live latents */
    const float *actions_in;       /* device float32 [rows, H, 2] raw (clamped), or NULL: the actor's own actions */
    float *reward, *value, *pcont; /* device float32 [rows, H], or NULL */
    float *returns, *weight;       /* device float32 [rows, H - 1], or NULL */
    float *actions;                /* device float32 [rows, H, 2], or NULL */
    float *features;               /* device float32 [rows, H, 230], or NULL */
    float *reward_start, *value_start, *pcont_start;      /* device float32 [rows], or NULL: the heads on the starting feature */
} rc_policy_returns_args;
/* rc_policy_returns: one launch on the handle's stream; rows = n_cars (live) or starts.  A pure function of its inputs: the agent's
 * state, RC_F_ACTION_IN, the arena, the episode log and every counter stay as they are.  RC_ERR_INVALID: wrong struct_size, no
 * policy loaded, the policy loaded without img2 / img3, no output asked for, value, returns or value_start without a value head,
 * reward, returns or reward_start without a reward head, pcont_start without a pcont head, horizon outside [0, 64] or too short
 * for the outputs asked for, unknown mode, lambda_ or discount not finite or outside [0, 1], state_in together with a non-zero mask
 * or starts outside [1, 2^31), live latents with an empty mask or bits beyond cars_per_env.  Kernels: rc_policy_returns_kernel,
 * rc_policy_returns_sampled_kernel, timed under RC_K_POLICY. */
int rc_policy_returns(rc_env *env, const rc_policy_returns_args *args);

/* The actor loss's gradient through the dream: the joint between rc_policy_returns, rc_policy_dream_grad and
 * rc_policy_actor_fit_step (the reference's actor_loss, dreamer/models.py:113-128; DESIGN.md §2 item 26;
 * tests/policy_returns_grad_spec.c is the CPU restatement, the device equals it bit for bit).  The forward is rc_policy_returns'
 * rollout - both modes, live latents or state_in, closed loop or under actions_in, the same draws and keys - and every forward output
 * it offers comes out byte for byte as rc_policy_returns gives it.  The objective of a row is
 *   J = sum over t < H - 1 of (scale * weight[t]) * returns[t]
 * with weight a constant (the reference's stop_gradient(cumprod)) and returns differentiated through reward, value and pcont (p is
 * the constant `discount`, without a gradient, where no pcont head is loaded); with scale = -1 / (rows * (H - 1)) the sum of J over
 * the rows is the reference's actor_loss.  The backward pass carries J's cotangent through the three heads and the prior step
 * (RSSM.img_step) for t = H - 1 .. 0, with respect to their inputs only.  The actor is NOT differentiated: the reference feeds it
 * stop_gradient(feat) (models.py:218-219), so its weights see the loss only through the action that enters img_step at each step -
 * what leaves here is that cotangent, with the actor's input and draw, as the rows rc_policy_actor_fit_step(grad_actions) takes.
 * Outputs, each optional, at least one of grad_actions and grad_state:
 *   grad_actions   [rows, H, 2]    dJ / d a_t, a_t the action that enters step t; under actions_in it is with respect to the raw
 *                                  action: exactly +0 where it lies outside [-1, 1] (bounds inclusive, as rc_policy_dream_grad)
 *   actor_features [rows, H, 230]  the feature the actor read for a_t: the start feature at t = 0, features[t - 1] after (stoch | deter)
 *   eps            [rows, H, 2]    the two normals of a_t's draw (block 8, words 0-1); mode SAMPLE in closed loop only
 *   grad_state     [rows, 230]     dJ / d (stoch | deter) of the start
 * A reward head and a value head must be loaded.  The activations of the forward are kept in a scratch the handle owns (4 648
 * floats per row and step, at most 1 GiB, grown on demand, released with the weights); the rows are cut into chunks of chunk_rows
 * (0: as many as the scratch's limit holds), one launch per chunk - the results do not depend on the chunking, the grid or the
 * shard.  No atomics and no reduction across rows.  A pure function of its inputs otherwise, as rc_policy_returns. */
typedef struct rc_policy_returns_grad_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_returns_grad_args) */
    int32_t horizon;               /* H in [2, RC_POLICY_IMAGINE_MAX_HORIZON] */
    int32_t mode;                  /* RC_POLICY_IMAGINE_* */
    uint32_t slot_mask;            /* live latents: bit a = slot a, as rc_policy_act's; with state_in: 0 */
    float lambda_;                 /* in [0, 1] */
    float discount;                /* in [0, 1]: the constant pcont when no pcont head is loaded */
    float scale;                   /* finite; the actor loss: -1 / (rows * (H - 1)) */
    uint32_t reserved;             /* 0 */
    uint64_t seed;
    int64_t starts;                /* with state_in: its rows, in [1, 2^31); live latents: 0 */
    uint64_t row_offset;           /* with state_in: the id of row 0 (mode SAMPLE) */
    int64_t chunk_rows;            /* rows per launch, rounded up to a multiple of 32; 0: derived from the scratch's limit */
    const float *state_in;         /* device float32 [starts, 232], or NULL: the live latents */
    const float *actions_in;       /* device float32 [rows, H, 2] raw (clamped), or NULL: the actor's own actions */
    float *reward, *value, *pcont; /* device float32 [rows, H], or NULL: as rc_policy_returns' */
    float *returns, *weight;       /* device float32 [rows, H - 1], or NULL */
    float *actions;                /* device float32 [rows, H, 2], or NULL */
    float *features;               /* device float32 [rows, H, 230], or NULL */
    float *reward_start, *value_start, *pcont_start;      /* device float32 [rows], or NULL */
    float *grad_actions;           /* device float32 [rows, H, 2], or NULL */
    float *actor_features;         /* device float32 [rows, H, 230], or NULL */
    float *eps;                    /* device float32 [rows, H, 2], or NULL */
    float *grad_state;             /* device float32 [rows, 230], or NULL */
} rc_policy_returns_grad_args;
/* rc_policy_returns_grad: one launch per chunk on the handle's stream.  RC_ERR_INVALID: wrong struct_size, no policy loaded, the
 * policy loaded without img2 / img3, no reward head, no value head, pcont_start without a pcont head, horizon outside [2, 64],
 * unknown mode, lambda_ or discount not finite or outside [0, 1], scale not finite, chunk_rows < 0, neither grad_actions nor
 * grad_state asked for, eps in mode MEAN or together with actions_in, state_in together with a non-zero mask or starts outside
 * [1, 2^31), starts != 0 with state_in NULL, live latents with an empty mask or bits beyond cars_per_env; nothing is launched on a
 * refusal.  Kernels: rc_policy_returns_grad_kernel, rc_policy_returns_grad_sampled_kernel (and, at the first call after a head was
 * loaded or fitted, rc_policy_dream_grad_transpose_kernel for its transposed images), timed under RC_K_POLICY. */
int rc_policy_returns_grad(rc_env *env, const rc_policy_returns_grad_args *args);

/* Fitting the critic on the device: the reference's value update (dreamer/models.py:129-137: value_loss = -mean(weight *
 * value(feat).log_prob(stop_gradient(returns))) under value_opt, which owns the value head's eight arrays alone; dreamer/tools.py:421-455
 * `Optimizer`: clip_by_global_norm, then Adam) - one MLP's forward pass, backward pass, global-norm clip and Adam on tensors that
 * rc_policy_returns leaves on the device (tests/policy_fit_spec.c is the CPU restatement of the whole fit engine, the device equals it
 * bit for bit).  The pcont head is the same network under a Bernoulli likelihood with soft targets (models.py:101-105).  With o the
 * head's output on features[i], t = target[i], w = weight[i] (1 where weight is NULL), N = rows:
 *   value   loss = -(1/N) sum w (-(o - t)^2 / 2 - log(2 pi) / 2)                       delta_o = w (o - t) / N
 *   pcont   loss = -(1/N) sum w (t log sigmoid(o) + (1 - t) log(1 - sigmoid(o)))       delta_o = w (sigmoid(o) - t) / N
 * The gradient's sum over the rows has a fixed order that depends on N alone (no atomics: two steps on the same inputs give the same
 * bits on any grid).  norm = sqrt(sum g^2) over the eight arrays; g <- g clip / max(norm, clip) (clip 0: no clipping); a step whose
 * norm is not finite changes nothing and does not count (the reference's LossScaleOptimizer skips it; the loss scale itself is the
 * identity under precision 32 and is not modelled).  Adam as TF's ResourceApplyAdam, t = the steps taken including this one:
 *   m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  w <- w - lr sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + epsilon)
 * (beta^t is a running product in binary64 kept with the moments on the device: a power from the host would have to know whether
 * the last step was skipped).  No weight decay (the reference's config has 0).  The new weights are written where rc_policy_returns
 * and every other reader of the critic find them; the other head, the policy, the latents, the arena and every counter stay as they are.
 *   rc_policy_fit_begin  opens the optimizer of one head (it must be loaded: rc_policy_load_critic): moments zero, step 0.  One per
 *                        head, both may be open; a second begin starts over.  rc_policy_load_critic, rc_policy_load and
 *                        rc_policy_unload close them.
 *   rc_policy_fit_step   one update, stream-ordered on the handle's stream, no synchronisation.  status, when given, receives
 *                        loss, grad_norm (before the clip), skipped (0 / 1) and the step count after this step.
 *   rc_policy_fit_end    frees the optimizer's state; the fitted weights stay loaded.
 *   rc_policy_read_critic copies the loaded heads back into the caller's host arrays (data pointers to [rows, cols] float32 of the
 *                        checkpoint's shapes, written despite the const; the pcont_* pointers may be NULL): the inverse of
 *                        rc_policy_load_critic's packing.  Synchronises the stream.
 * RC_ERR_INVALID: wrong struct_size, unknown head, the head not loaded (begin), no optimizer open for the head (step), features or
 * target NULL, rows outside [1, 2^31), a hyper-parameter negative or not finite, a beta outside [0, 1); read_critic: no critic
 * loaded, a wrong shape, pcont_* asked for without a pcont head.  Kernels: rc_policy_fit_rows_kernel, rc_policy_fit_wgrad_kernel,
 * rc_policy_fit_sums_kernel, rc_policy_fit_scale_kernel, rc_policy_fit_apply_kernel (and rc_policy_fit_transpose_kernel in begin),
 * timed together under RC_K_POLICY.
 *
 * The reward head (RC_POLICY_FIT_REWARD; DESIGN.md §2 item 24, tests/policy_fit_spec.c at depth 2 is the CPU restatement, the device
 * equals it bit for bit): the same engine at two hidden layers, on the arrays rc_policy_load_heads loaded - DenseDecoder((), 2, 400),
 * 230 -> 400 -> 400 -> 1, under the value head's Normal(o, 1) likelihood: loss and delta_o as "value" above, target = the recorded
 * reward.  The reference trains this term inside its model loss under model_opt (dreamer/models.py:97-110, 135, 167-181), where its gradient also
 * reaches the RSSM and the encoder; here the head's six arrays move and nothing else.  The gradient is [231][400] | [401][400] |
 * [401][1] = 253 201 elements in the same fixed order, the rest (sum tree, skip, clip, Adam) is unchanged.  The new weights are
 * written where rc_policy_imagine, rc_policy_observe, rc_policy_dream_ahead, rc_policy_returns and rc_policy_dream_grad read them
 * (the last keeps transposed copies: its next call makes them again on the stream); the critic, the policy, the latents, the arena
 * and every counter stay as they are.  Its optimizer is independent of the critic's two: rc_policy_load_heads, rc_policy_load and
 * rc_policy_unload close it, rc_policy_load_critic does not (and rc_policy_load_heads leaves the critic's open).  begin without a
 * loaded reward head is RC_ERR_INVALID.  Kernels: rc_policy_fit_reward_rows_kernel in place of rc_policy_fit_rows_kernel, the other
 * four as above.
 *   rc_policy_read_heads  copies the loaded reward head back into the caller's host arrays (data pointers to [rows, cols] float32 of
 *                        the checkpoint's shapes, written despite the const): the inverse of rc_policy_load_heads' packing.
 *                        Synchronises the stream.  RC_ERR_INVALID: wrong struct_size, no reward head loaded, an array missing or
 *                        of a wrong shape. */
#define RC_POLICY_FIT_VALUE 0
#define RC_POLICY_FIT_PCONT 1
#define RC_POLICY_FIT_REWARD 2
typedef struct rc_policy_fit_config {
    uint32_t struct_size;          /* = sizeof(rc_policy_fit_config) */
    int32_t head;                  /* RC_POLICY_FIT_* */
} rc_policy_fit_config;
typedef struct rc_policy_fit_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_fit_args) */
    int32_t head;                  /* RC_POLICY_FIT_* */
    int64_t rows;                  /* N in [1, 2^31) */
    const float *features;         /* device float32 [rows, 230] = stoch | deter */
    const float *target;           /* device float32 [rows] */
    const float *weight;           /* device float32 [rows], or NULL: all 1 */
    float lr, clip;                /* the reference's value_lr 8e-5 (the reward head: model_lr 6e-4) and grad_clip 1.0 (dream.py:85-88); clip 0: none */
    float beta1, beta2, epsilon;   /* TF's 0.9, 0.999, 1e-7 */
    float *status;                 /* device float32 [4] = loss, grad_norm, skipped, step; or NULL */
} rc_policy_fit_args;
int rc_policy_fit_begin(rc_env *env, const rc_policy_fit_config *cfg);
int rc_policy_fit_step(rc_env *env, const rc_policy_fit_args *args);
int rc_policy_fit_end(rc_env *env, int32_t head);
int rc_policy_read_critic(rc_env *env, rc_policy_critic *out);
int rc_policy_read_heads(rc_env *env, rc_policy_heads *out);

/* Fitting the actor on the device: the actor's own backward pass and optimizer on the fit engine (RC_POLICY_FIT_ACTOR; DESIGN.md §2
 * item 25, tests/policy_actor_fit_spec.c - the actor's rule on policy_fit_spec.c's engine - is the CPU restatement, the device equals it bit for bit).  The network is the reference's
 * plain ActionDecoder(2, 4, 400, 'tanh_normal'), 230 -> 400 -> 400 -> 400 -> 400 -> 4, ELU, init_std 5, min_std 1e-4, mean_scale 5
 * (dreamer/models.py:535-560); the optimizer is actor_opt's: lr 8e-5, clip 1.0 (dreamer/dream.py:87-88), dreamer/tools.py:421-455 as
 * for the critic.  The closed-loop gradient through the dream (the reference's actor_loss) is NOT computed here: the caller supplies
 * the gradient with respect to the actions, or target actions.  Per row q of N, with o[0..3] the output layer on features[q], e =
 * eps[q] (NULL: the mode action, u = mu), w = weight[q] (NULL: 1):
 *   mu_j = 5 tanh(o_j / 5);  sd_j = softplus(o_{2+j} + raw_init_std) + 1e-4;  u_j = fmaf(sd_j, e_j, mu_j);  act_j = tanh(u_j)
 *   target  loss = (1/N) sum w 0.5 sum_j (act_j - target_j)^2        ga_j = w (act_j - target_j) / N
 *   grad    loss = 0 (the caller owns it)                            ga_j = w grad_j
 *   du_j = ga_j (1 - act_j^2);  delta o_j = du_j (1 - tanh(o_j / 5)^2);  delta o_{2+j} = du_j e_j sigmoid(o_{2+j} + raw_init_std)
 * then back through the four hidden layers as the critic's fit does, and, when asked for, grad_features = delta1 W0^T.  The gradient
 * is [231][400] | 3 x [401][400] | [401][4] = 575 204 elements in the critic's fixed order; sum tree, skip, clip and Adam are the
 * critic's.  The new weights are written into every image of the actor that a kernel reads: rc_policy_act (all three modes),
 * rc_policy_imagine and rc_policy_returns read the fitted actor at their next call, with no reload and no latent reset; the RSSM,
 * the heads, the latents, the arena and every counter stay as they are.  Actions are raw, in [-1, 1]: RC_F_ACTION_IN's convention
 * under remap_actions.
 *   rc_policy_fit_begin / rc_policy_fit_end  with RC_POLICY_FIT_ACTOR open and free the optimizer.  rc_policy_load, rc_policy_unload,
 *                        rc_policy_load_actor and rc_destroy close it.  A "normalized" actor (hnorm_* arrays: batch statistics in
 *                        training) is refused.
 *   rc_policy_actor_fit_step  one update, stream-ordered, no synchronisation; status as rc_policy_fit_step's.
 *   rc_policy_actor_forward   the forward pass alone on given features: action, mean (mu), std (sd), each [rows, 2] or NULL.  With eps
 *                        NULL the action is byte-identical to what rc_policy_act writes in mode mean for the same feature.
 *   rc_policy_read_actor copies the actor's ten arrays back into the caller's host arrays (data pointers to [rows, cols] float32 of
 *                        the checkpoint's shapes, written despite the const).  Synchronises the stream.
 *   rc_policy_load_actor replaces the actor's ten arrays alone, in every image; closes the actor's optimizer and resets nothing else.
 * RC_ERR_INVALID: wrong struct_size, no policy loaded, a normalized actor, no optimizer open (step), both or neither of target and
 * grad, rows outside [1, 2^31), features NULL, no output asked for (forward), a hyper-parameter negative or not finite, a beta
 * outside [0, 1), an array missing or of a wrong shape (read, load).  Kernels: rc_policy_fit_actor_rows_kernel in place of
 * rc_policy_fit_rows_kernel, the other four as for the critic; rc_policy_actor_forward_kernel; timed under RC_K_POLICY. */
#define RC_POLICY_FIT_ACTOR 3
typedef struct rc_policy_actor_fit_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_actor_fit_args) */
    int64_t rows;                  /* N in [1, 2^31) */
    const float *features;         /* device float32 [rows, 230] = stoch | deter */
    const float *eps;              /* device float32 [rows, 2], or NULL: the mode action */
    const float *weight;           /* device float32 [rows], or NULL: all 1 */
    const float *target;           /* device float32 [rows, 2] raw actions, or NULL ... */
    const float *grad;             /* ... device float32 [rows, 2] the gradient with respect to the actions: exactly one of the two */
    float *grad_features;          /* device float32 [rows, 230], or NULL */
    float lr, clip;                /* the reference's actor_lr 8e-5 and grad_clip 1.0 (dreamer/dream.py:87-88); clip 0: none */
    float beta1, beta2, epsilon;   /* TF's 0.9, 0.999, 1e-7 */
    float *status;                 /* device float32 [4] = loss, grad_norm, skipped, step; or NULL */
} rc_policy_actor_fit_args;
typedef struct rc_policy_actor_forward_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_actor_forward_args) */
    int64_t rows;                  /* in [1, 2^31) */
    const float *features;         /* device float32 [rows, 230] */
    const float *eps;              /* device float32 [rows, 2], or NULL */
    float *action, *mean, *std;    /* device float32 [rows, 2] each; any may be NULL, not all */
} rc_policy_actor_forward_args;
typedef struct rc_policy_actor {   /* the ActionDecoder's arrays (dreamer/models.py:535-560), rc_policy_weights' of the same names */
    uint32_t struct_size;          /* = sizeof(rc_policy_actor) */
    rc_policy_array h0_w, h0_b, h1_w, h1_b, h2_w, h2_b, h3_w, h3_b;      /* [230, 400], [400]; 3 x ([400, 400], [400]) */
    rc_policy_array hout_w, hout_b;                                      /* [400, 4], [4]: mean 0, mean 1, raw std 0, raw std 1 */
} rc_policy_actor;
int rc_policy_actor_fit_step(rc_env *env, const rc_policy_actor_fit_args *args);
int rc_policy_actor_forward(rc_env *env, const rc_policy_actor_forward_args *args);
int rc_policy_read_actor(rc_env *env, rc_policy_actor *out);
int rc_policy_load_actor(rc_env *env, const rc_policy_actor *actor);

/* Recorded sequences: the posterior chain over N recorded windows of T scans and actions (DESIGN.md §2 item 17;
 * tests/policy_observe_spec.c is the CPU restatement, the device equals it bit for bit) - dreamer/models.py:325-336 RSSM.observe,
 * the operation the reference runs on every replay batch: `post, prior = observe(embed, action)`, kl_divergence(post, prior) and the
 * reward likelihood of dreamer/models.py:84-110 `_train`, and the "observe 5, imagine the rest" of models.py:243-277
 * `_image_summaries` and dreamer/evaluations/produce_reconstruction.py:36-57.  A row is one window, not a car of the env.
 * For t = 0 .. length - 1 from the start state: the prior step img_step under a_t = clamp(actions[row, t], -1, 1) - the action
 * recorded WITH scan t, the one that led to it, as the reference's episodes store it (a window's first row after a reset carries
 * action 0) -; for t < context the posterior step obs_step on scan[row, t] (metres; clip to [0, 15] / 15 - 0.5 as rc_policy_act).
 * stoch' comes from the posterior for t < context and from the prior after it: context = length is RSSM.observe, context = K <
 * length is observe(..[:K]) followed by RSSM.imagine(action[K:], last post) in one call.
 *   RC_POLICY_OBSERVE_MEAN     stoch' = the mean: deterministic, what rc_policy_act's default mode computes step by step.
 *   RC_POLICY_OBSERVE_SAMPLE   stoch' ~ Normal(mean, std), Philox4x32-10 keyed by `seed` and counted by (row_offset + row, t, index):
 *                              not by N, the workgroup or the call history - two shards with their row_offset give the whole batch.
 * Outputs at [row, t], each optional: features = [stoch', deter'], prior_mean / prior_std, reward = the reward head on the feature;
 * for t < context also post_mean / post_std and kl = KL(post || prior) summed over the 30 dimensions (entries at t >= context are
 * not written).  std = softplus(raw) + 0.1.  state_in: [rows, 232] = stoch | deter | (2 columns that are not read), NULL =
 * RSSM.initial's zeros; state_out: the last stoch' | deter' | a_{T-1}, in rc_policy_state's layout.  A pure function of its inputs:
 * the agent's state, RC_F_ACTION_IN, the arena and every counter stay as they are (unless the caller passes rc_policy_state's
 * memory as state_out, after which rc_policy_act / rc_policy_imagine go on from there). */
#define RC_POLICY_OBSERVE_MEAN 0
#define RC_POLICY_OBSERVE_SAMPLE 1
#define RC_POLICY_OBSERVE_MAX_LENGTH 64
typedef struct rc_policy_observe_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_observe_args) */
    int32_t length;                /* T in [1, RC_POLICY_OBSERVE_MAX_LENGTH]; the reference's batch_length is 50 */
    int32_t context;               /* in [1, length]: the steps that see their scan */
    int32_t mode;                  /* RC_POLICY_OBSERVE_* */
    int64_t rows;                  /* N >= 1 */
    uint64_t seed;
    uint64_t row_offset;           /* row id of row 0 (mode SAMPLE) */
    const float *scan;             /* device float32 [rows, T, 1080], metres */
    const float *actions;          /* device float32 [rows, T, 2], raw in [-1, 1] (clamped) */
    const float *state_in;         /* device float32 [rows, 232], or NULL */
    float *features;               /* device float32 [rows, T, 230], or NULL */
    float *post_mean, *post_std;   /* device float32 [rows, T, 30], or NULL; written for t < context */
    float *prior_mean, *prior_std; /* device float32 [rows, T, 30], or NULL */
    float *kl;                     /* device float32 [rows, T], or NULL; written for t < context */
    float *reward;                 /* device float32 [rows, T], or NULL */
    float *state_out;              /* device float32 [rows, 232], or NULL */
} rc_policy_observe_args;
/* rc_policy_observe: one launch for all rows and steps, on the handle's stream.  RC_ERR_INVALID: wrong struct_size, no policy
 * loaded, the policy loaded without img2 / img3, rows outside [1, 2^31), length outside [1, 64], context outside [1, length],
 * unknown mode, scan or actions NULL, no output asked for, reward asked for without a loaded head.  Kernels:
 * rc_policy_observe_kernel, rc_policy_observe_sampled_kernel, timed under RC_K_POLICY. */
int rc_policy_observe(rc_env *env, const rc_policy_observe_args *args);

/* The observation decoder: what the world model believes the car sees (tests/policy_decode_spec.c is the CPU
 * restatement, the device equals it bit for bit).  The reference's LidarOccupancyDecoder (dreamer/models.py:444-465) on a feature
 * [stoch 30 | deter 200]: dense 230 -> 64, then Conv2DTranspose(32, 5), (16, 5), (8, 6), (1, 6), all stride 2, 'valid', ReLU -
 * 1 x 1 -> 5 -> 13 -> 30 -> 64 pixels.  logits = the Bernoulli logits (>= 0: the last layer has a ReLU too), image = the
 * distribution's mode, logit > 0, in the encoding of RC_F_OCCUPANCY (1 = drivable).  It is what dreamer/models.py:243-277
 * `_image_summaries` and dreamer/evaluations/produce_reconstruction.py:36-57 draw: on the live latent the reconstruction, on the
 * features of rc_policy_imagine the open-loop prediction.
 *
 * rc_policy_decoder: the decoder's ten arrays, host pointers as in rc_policy_weights; a kernel [kh, kw, out, in] is passed
 * C-contiguous with rows = kh kw out, cols = in.  rc_policy_load_decoder checks the shapes first (RC_ERR_INVALID names the first
 * that is wrong), needs a loaded policy and copies the arrays; d = NULL drops the decoder, and so do rc_policy_load and
 * rc_policy_unload. */
typedef struct rc_policy_decoder {
    uint32_t struct_size;          /* = sizeof(rc_policy_decoder) */
    rc_policy_array dec_h1_w, dec_h1_b;                        /* [230, 64], [64]     input [stoch, deter]                     */
    rc_policy_array dec_h2_k, dec_h2_b;                        /* [5 5 32, 64] = [800, 64], [32]                               */
    rc_policy_array dec_h3_k, dec_h3_b;                        /* [5 5 16, 32] = [400, 32], [16]                               */
    rc_policy_array dec_h4_k, dec_h4_b;                        /* [6 6 8, 16] = [288, 16], [8]                                 */
    rc_policy_array dec_h5_k, dec_h5_b;                        /* [6 6 1, 8] = [36, 8], [1]                                    */
} rc_policy_decoder;
int rc_policy_load_decoder(rc_env *env, const rc_policy_decoder *d);
#define RC_POLICY_DECODE_IMAGE 64  /* the decoded image is 64 x 64, as RC_F_OCCUPANCY */
typedef struct rc_policy_decode_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_decode_args) */
    const float *features;         /* device float32 [rows, 230], or NULL: the live latents of rc_policy_state, one row per car */
    int64_t rows;                  /* with features: >= 1; ignored without */
    uint32_t slot_mask;            /* live latents only: bit a = slot a, as rc_policy_act's; with features it must be 0 */
    float *logits;                 /* device float32 [rows, 64, 64], or NULL */
    uint8_t *image;                /* device uint8 [rows, 64, 64], or NULL */
    int32_t *mismatch;             /* device int32 [n_cars], or NULL; live latents only: the number of pixels in which the image
                                      differs from the car's RC_F_OCCUPANCY in the current arena (obs_type RC_OBS_LIDAR_OCCUPANCY or
                                      RC_OBS_LIDAR_OCCUPANCY_REFERENCE); computed whether or not `image` is asked for */
} rc_policy_decode_args;
/* rc_policy_decode: one launch on the handle's stream.  A pure function of its input: the agent's state, RC_F_ACTION_IN, the arena
 * and every counter stay as they are.  Live latents: rows are indexed by car, rows of cars outside the mask are not touched.
 * RC_ERR_INVALID: wrong struct_size, no policy loaded, no decoder loaded, no output asked for, rows < 1 or a slot mask with
 * features, an empty mask or bits beyond cars_per_env without, mismatch with features or under obs_type RC_OBS_LIDAR.
 * Kernel: rc_policy_decode_kernel, timed under RC_K_POLICY. */
int rc_policy_decode(rc_env *env, const rc_policy_decode_args *args);

/* rc_policy_decode_loglik: rc_policy_decode with the Bernoulli log-likelihood of a target image, `image_pred.log_prob(
 * data['lidar_occupancy'])` of dreamer/models.py:99 (tests/policy_decode_loglik_spec.c fixes the order of
 * summation, the device equals it bit for bit): loglik = sum over the 64 x 64 pixels of x logit - softplus(logit), x = 1 where the
 * target's byte is not 0.  A second instantiation of the same kernel body; rc_policy_decode and its args are as they were. */
typedef struct rc_policy_decode_loglik_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_decode_loglik_args) */
    const float *features;         /* device float32 [rows, 230], or NULL: the live latents, one row per car */
    int64_t rows;                  /* with features: >= 1; ignored without */
    uint32_t slot_mask;            /* live latents only; with features it must be 0 */
    const uint8_t *target;         /* with features: device uint8 [rows, 64, 64] on a 2-byte boundary, or NULL (then no loglik); live
                                      latents: must be NULL - the target is the car's own RC_F_OCCUPANCY in the current arena */
    float *loglik;                 /* device float32 [rows], or NULL */
    float *logits;                 /* device float32 [rows, 64, 64], or NULL: as rc_policy_decode's */
    uint8_t *image;                /* device uint8 [rows, 64, 64], or NULL: as rc_policy_decode's */
} rc_policy_decode_loglik_args;
/* One launch on the handle's stream, pure as rc_policy_decode.  RC_ERR_INVALID: wrong struct_size, no policy loaded, no decoder
 * loaded, no output asked for, rows < 1 or a slot mask with features, loglik with features and no target, an empty mask or bits
 * beyond cars_per_env without features, a target with live latents, loglik on live latents under obs_type RC_OBS_LIDAR.
 * Kernel: rc_policy_decode_loglik_kernel, timed under RC_K_POLICY. */
int rc_policy_decode_loglik(rc_env *env, const rc_policy_decode_loglik_args *args);

/* The LiDAR distance decoder: what scan the world model expects (tests/policy_lidar_decode_spec.c is the CPU
 * restatement, the device equals it bit for bit).  The reference's LidarDistanceDecoder (dreamer/models.py:424-441), the decoder of
 * obs_type `lidar`, on a feature [stoch 30 | deter 200]: dense1 230 -> 256 (no activation), dense2 256 -> 512 (ReLU), params
 * 512 -> 2160 (leaky ReLU, slope 0.2), then tfpl.IndependentNormal(1080): loc = the first 1080 outputs, scale = softplus of the
 * last 1080, both in the model's units scan_m / 15 - 0.5.  loglik = sum over the beams b of
 * -((y_b - loc_b) / scale_b)^2 / 2 - log(scale_b) - log(2 pi) / 2 with y = the target scan, clipped to [0, 15] m and brought to the
 * model's units on the device, in the order of summation the spec fixes: `image_pred.log_prob(data['lidar'])` of
 * dreamer/models.py:99.  No shipped checkpoint carries this decoder: the caller brings the six arrays (host pointers as in
 * rc_policy_weights).  rc_policy_load_lidar_decoder checks the shapes first (RC_ERR_INVALID names the first that is wrong), needs a
 * loaded policy and copies the arrays; d = NULL drops the decoder, and so do rc_policy_load and rc_policy_unload. */
typedef struct rc_policy_lidar_decoder {
    uint32_t struct_size;          /* = sizeof(rc_policy_lidar_decoder) */
    rc_policy_array ldec_dense1_w, ldec_dense1_b;              /* [230, 256], [256]   input [stoch, deter]                     */
    rc_policy_array ldec_dense2_w, ldec_dense2_b;              /* [256, 512], [512]                                            */
    rc_policy_array ldec_params_w, ldec_params_b;              /* [512, 2160], [2160] columns: loc 1080, then raw scale 1080   */
} rc_policy_lidar_decoder;
int rc_policy_load_lidar_decoder(rc_env *env, const rc_policy_lidar_decoder *d);
typedef struct rc_policy_decode_lidar_args {
    uint32_t struct_size;          /* = sizeof(rc_policy_decode_lidar_args) */
    const float *features;         /* device float32 [rows, 230], or NULL: the live latents of rc_policy_state, one row per car */
    int64_t rows;                  /* with features: >= 1; ignored without */
    uint32_t slot_mask;            /* live latents only: bit a = slot a, as rc_policy_act's; with features it must be 0 */
    const float *target;           /* with features: device float32 [rows, 1080] in metres, or NULL (then no loglik); live latents:
                                      must be NULL - the target is the car's own RC_F_LIDAR in the current arena */
    float *mean;                   /* device float32 [rows, 1080], or NULL: loc, the distribution's mode */
    float *std;                    /* device float32 [rows, 1080], or NULL: scale */
    float *loglik;                 /* device float32 [rows], or NULL */
} rc_policy_decode_lidar_args;
/* rc_policy_decode_lidar: one launch on the handle's stream.  A pure function of its input: the agent's state, RC_F_ACTION_IN, the
 * arena and every counter stay as they are.  Live latents: rows are indexed by car, rows of cars outside the mask are not touched.
 * RC_ERR_INVALID: wrong struct_size, no policy loaded, no LiDAR decoder loaded, no output asked for, rows < 1 or a slot mask with
 * features, loglik with features and no target, an empty mask or bits beyond cars_per_env without features, a target with live
 * latents, loglik on live latents under a lidar_transform other than RC_LIDAR_METRES.
 * Kernel: rc_policy_decode_lidar_kernel, timed under RC_K_POLICY. */
int rc_policy_decode_lidar(rc_env *env, const rc_policy_decode_lidar_args *args);

/* ---- Episode log: return, length, progress and time of every episode, kept on the device (opt-in; off = the launches of a step
 * are what they are without it) ---------------------------------------------------------------------------------------------------
 * What the reference computes on the host from each recorded episode (dreamer/callbacks.py:56-100, summarize_episode /
 * summarize_eval_episode: return = reward.sum(), length = len(reward) - 1, progress = max(progress), time = max(time)) and
 * what dreamer/evaluations/run_evaluation.py:43-64 loops over.  With auto_reset the terminal reward, progress and time of an
 * env are in the arena for exactly one call; the log sums them per car in handle-owned device memory and appends one
 * rc_episode_row per car in the call in which the env's episode ends.  No host round trip; rc_arena_bytes, the trajectory
 * slab, the compact record and RC_ABI_VERSION do not change.
 *
 * An episode is an ENV's: it ends for all its cars in the call in which any car's RC_F_DONE becomes 1 (that is how the env is
 * reset, and how the reference's Collect fires, dreamer/wrappers.py:221-226).  Per car, over the rc_step / rc_step_random /
 * rc_step_group calls of the episode (one call = one agent step = one Collect transition), from the values the call leaves in
 * the CURRENT arena (rc_set_arena) - the terminal values on the last call, also under auto-reset:
 *   env       global env id (first_env + index in the handle): does not depend on the sharding
 *   slot      car slot 0 .. cars_per_env - 1
 *   track     the track the episode was DRIVEN on: the track-set id latched when the episode started (after an auto-reset
 *             rc_track_ids already names the next one); 0 without a track set
 *   episode   ordinal of the episode among this env's episodes that ended since enable / clear (dropped and skipped ones count), from 0
 *   call      index of the step call, counted since enable / clear, in which it ended
 *   length    calls in the episode = the reference's len(reward) - 1
 *   ret       binary32 sum of RC_F_REWARD in call order, starting from +0.0f (the reset row adds 0)
 *   progress  max over -1.0f (the reset row, wrappers.py:232-236) and every call's RC_F_PROGRESS_TOTAL
 *   time      max over 0.0f and every call's RC_F_TIME
 *   laps      terminal RC_F_LAP - 1
 *   flags     bit 0 terminal wall collision, 1 terminal opponent collision, 2 truncated (RC_F_TRUNCATED), 3 wrong_way seen in any
 *             call of the episode, 4 this car's own done was set (0 = the episode ended because a team-mate's did)
 * Rules:
 *   - an episode is logged ONCE.  Without auto_reset a finished env is frozen and keeps done = 1 in every later call: no second
 *     row and no further sums until it is reset.
 *   - rc_reset (with or without a mask) of an env whose episode is running discards its sums without a row and adds 1 to
 *     `abandoned` (one per env, whatever cars_per_env; a reset right after a reset abandons an episode of length 0).
 *     rc_set_pose changes nothing in the log.
 *   - the log follows an env from its next reset on - rc_reset or the auto-reset inside a step: enabled in the middle of an
 *     episode it logs nothing for that partial episode.
 *   - rows are ordered by call, then env, then slot - strictly, not up to a permutation: two runs with the same seeds give
 *     byte-identical row buffers.
 *   - capacity is fixed at enable.  A row that does not fit is counted in `dropped`; rows already written are never
 *     overwritten (not a ring: the first k episodes of every env survive).  max_episodes > 0 is a quota per env: an episode
 *     whose ordinal is >= the quota gets no rows, its cars are counted in `skipped`, and `envs_at_quota` counts the envs whose
 *     ordinal has reached the quota - one integer to poll for "every env has finished max_episodes episodes", after which the log
 *     holds exactly n_cars * max_episodes rows if the capacity allows.
 *   - counters: uint64 [6] in device memory = written, dropped, skipped (rows), abandoned (episodes), envs_at_quota (envs), calls.
 * rc_episode_log_enable allocates; called again it clears and, if the capacity differs, reallocates the rows (running episodes keep
 * their sums).  rc_episode_log gives the device pointers: the rows (capacity_rows x 48 bytes, the first `written` valid) and the
 * counters.  rc_episode_log_clear: rows, counters and ordinals to zero, `call` restarts at 0, running episodes keep their sums.
 * rc_episode_log_disable frees everything (synchronises the handle's stream).  In a group launch each handle keeps its own log.
 * RC_ERR_INVALID: env NULL, capacity_rows < 1, max_episodes < 0, rc_episode_log / rc_episode_log_clear before enable.
 * Kernels: rc_episode_count_kernel + rc_episode_update_kernel behind every step's dynamics launch, rc_episode_reset_kernel behind
 * rc_reset's.  They have no RC_K_* timer; while rc_set_profiling is on, rc_episode_log_time reports the summed time between two
 * events around the log's launches of every step (and their number); rc_reset_kernel_times zeroes it. */
typedef struct rc_episode_row {
    int32_t  env, slot, track;
    uint32_t episode, call;
    int32_t  length;
    float    ret, progress, time;
    int32_t  laps;
    uint32_t flags, reserved;      /* reserved = 0 */
} rc_episode_row;                  /* 48 bytes */
enum { RC_EP_WALL = 1, RC_EP_OPPONENT = 2, RC_EP_TRUNCATED = 4, RC_EP_WRONG_WAY = 8, RC_EP_OWN_DONE = 16 };   /* rc_episode_row.flags */
int rc_episode_log_enable(rc_env *env, int64_t capacity_rows, int32_t max_episodes);
int rc_episode_log_disable(rc_env *env);
int rc_episode_log(rc_env *env, void **rows_dev, size_t *capacity_rows, void **counters_dev, size_t *counters_bytes);
int rc_episode_log_clear(rc_env *env);
int rc_episode_log_time(rc_env *env, double *total_ms, uint64_t *launches);

/* ---- Look ahead in the simulator: what would really happen from here under these actions?
 * rc_look_ahead carries, for every env e, `candidates` action sequences of `horizon` agent steps through the env's true
 * dynamics, each from the env's live state as the last rc_step* / rc_reset / rc_set_pose left it (the cars, steps and
 * agent_steps, the n_step_progress windows, the cars' vehicle parameters while randomization is on, the env's current track
 * of a track set).  Every step applies exactly what rc_step(actions, repeat) applies on a handle with auto_reset = 0 - the
 * action convention, `repeat` sub-steps, wall and car-car collision, progress / lap / checkpoint, the slot's reward, done, the
 * break on the finishing sub-step, time_limit_steps - with the operations of the step's own kernel, bit for bit.  A finished
 * env is frozen, whether it finished before the call or inside the horizon: every later step has reward +0.0f and unchanged
 * flags; the look-ahead never resets, whatever the handle's auto_reset.  No random draw is involved.
 *   The call is pure: it reads the simulator's state and writes nothing but the arrays given here - no state array, no arena
 * section (RC_F_ACTION_IN included), not the live n_step_progress windows (each rollout carries a private copy), not the
 * episode log, its counters or the agent's latent.
 *   actions: float [E, K, H, A, 2] in device memory, C-contiguous (E = num_envs, K = candidates, H = horizon, A = cars_per_env),
 * in rc_step's convention.  Outputs, device memory, each optional (NULL), at least one required:
 *   reward       float   [E, K, H, A]     the step's reward
 *   flags        uint8   [E, K, H, A]     RC_LA_DONE | RC_LA_TRUNCATED | RC_LA_WALL | RC_LA_OPPONENT | RC_LA_WRONG_WAY after step t
 *   ret          float   [E, K, A]        binary32 sum of the H rewards in step order from +0.0f
 *   length       int32   [E, K]           steps taken until the env finished, the finishing step counted; H if it did not; 0 if it was
 *   final_state  float   [E, K, A, 8]     x, y, theta, v, delta, omega, (lap - 1) + progress, time
 *   pose         float   [E, K, H, A, 3]  x, y, theta after step t
 * One launch on the handle's stream (rc_look_ahead_kernel, one lane per (env, candidate)).  RC_ERR_NEEDS_RESET before the first
 * reset.  RC_ERR_INVALID: wrong struct_size, candidates < 1, horizon outside [1, RC_LOOK_AHEAD_MAX_HORIZON], repeat < 1,
 * E K beyond int32, actions NULL, no output asked for.  It has no RC_K_* timer: while rc_set_profiling is on,
 * rc_look_ahead_time reports the summed time of its launches (and their number); rc_reset_kernel_times zeroes it. */
#define RC_LOOK_AHEAD_MAX_HORIZON 64
enum { RC_LA_DONE = 1, RC_LA_TRUNCATED = 2, RC_LA_WALL = 4, RC_LA_OPPONENT = 8, RC_LA_WRONG_WAY = 16 };   /* flags */
typedef struct rc_look_ahead_args {
    uint32_t struct_size;          /* = sizeof(rc_look_ahead_args) */
    int32_t candidates, horizon, repeat;
    const float *actions;
    float *reward;
    uint8_t *flags;
    float *ret;
    int32_t *length;
    float *final_state;
    float *pose;
} rc_look_ahead_args;
int rc_look_ahead(rc_env *env, const rc_look_ahead_args *args);
int rc_look_ahead_time(rc_env *env, double *total_ms, uint64_t *launches);

int rc_get(rc_env *env, int32_t field, void **dev_ptr, size_t *bytes);
int rc_copy_out(rc_env *env, int32_t field, void *host_dst, size_t bytes);
/* The trajectory record of the last step as one contiguous device slab (fields LIDAR..TIME,
 * plus OCCUPANCY when enabled): the source buffer of the multi-GPU all-gather. */
int rc_trajectory_slab(rc_env *env, void **dev_ptr, size_t *bytes);

/* Device memory for clients that do not link the HIP runtime themselves (a plain-C learner process): allocation on the
 * handle's device, release, and a stream-ordered copy of caller-chosen device bytes to the host.  What they hand out
 * is ordinary device memory: usable as compact slab, gather destination or arena. */
int rc_device_alloc(rc_env *env, size_t bytes, void **dev_ptr);
int rc_device_free(rc_env *env, void *dev_ptr);
int rc_copy_from_device(rc_env *env, const void *dev_src, void *host_dst, size_t bytes);

/* ---- Half-size record and multi-GPU gather -------------------------------------------------------
 * The record of a step is 4 396 B per car, 4 320 of them the fp32 LiDAR row.  rc_set_compact_slab makes the scan
 * store a second copy of the row as uint16 - q = rne((v + off) * scale) with (off, scale) = (0, 65535/15) for
 * RC_LIDAR_METRES, (0.5, 65535) for RC_LIDAR_DREAMER, (0, 65535) for RC_LIDAR_UNIT: 0.23 mm per count, below the
 * 0.05 m map cell by two orders of magnitude - into a caller-owned device buffer, followed by a copy of the arena's
 * POSE..TIME sections (76 B per car): 2 236 B per car, the payload of RC_GATHER_FULL_U16.  Layout of the buffer:
 * uint16 [n][1080], padding to 64 B, then the POSE..TIME sections exactly as they lie in the arena
 * (rc_compact_layout gives the offsets).  NULL switches it off.  Alternate two buffers to overlap a gather with
 * the next step. */
size_t rc_compact_bytes(const rc_config *cfg);
int rc_set_compact_slab(rc_env *env, void *slab, size_t bytes);
int rc_compact_layout(rc_env *env, size_t *lidar_u16_bytes, size_t *summary_offset, size_t *summary_bytes);

/* The communicator: one rank per handle (= per GPU).  Rank 0 calls rc_comm_unique_id and hands the 128 bytes to the
 * other ranks by any means (file, socket, MPI, torch.distributed store); every rank then calls rc_comm_init.  RCCL is
 * bound at run time: the first of librccl.so.1 / librccl.so / /opt/rocm/lib that is already loaded in the process or
 * can be loaded, or the path given to rc_comm_library before the first use. */
int rc_comm_library(const char *path);
int rc_comm_unique_id(void *out_128_bytes, size_t bytes);
int rc_comm_init(rc_env *env, const void *unique_id, size_t bytes, int32_t rank, int32_t world);
int rc_comm_count(rc_env *env, int32_t *ranks);      /* ncclCommCount of the handle's communicator */

/* All-gather of the last step's record over the communicator: dev_dst receives world x rc_gather_bytes(mode) bytes,
 * rank r's record at r * rc_gather_bytes(mode).  RC_GATHER_FULL = the rc_trajectory_slab bytes (fp32 LiDAR),
 * RC_GATHER_FULL_U16 = the compact slab, RC_GATHER_SUMMARY = POSE..TIME only (the scans stay on their GPU).
 * Asynchronous: queued behind the work already on the handle's stream, runs on a stream of its own so that the next
 * steps overlap it - the caller must not let them overwrite the source (rc_set_arena / rc_set_compact_slab to the
 * other buffer of a pair) nor reuse dev_dst before rc_gather_wait.  rc_gather_wait orders the handle's stream behind
 * the collective; with host_sync != 0 it also blocks the host until the gathered bytes are there. */
enum { RC_GATHER_FULL = 0, RC_GATHER_FULL_U16 = 1, RC_GATHER_SUMMARY = 2 };
size_t rc_gather_bytes(rc_env *env, int32_t mode);
int rc_gather_trajectory(rc_env *env, int32_t mode, void *dev_dst, size_t dst_bytes);
int rc_gather_wait(rc_env *env, int32_t host_sync);

/* ---- The same all-gather as DIRECT PEER COPIES (on the xGMI full mesh each rank's record should cross
 * each link once - N - 1 concurrent copies into the peers' buffers - where a ring passes it on N - 1 times).  No RCCL:
 * hipIpc memory handles, one copy stream per peer, sequence flags in uncached device memory.
 *   rc_p2p_setup    allocates this rank's destination - two slots of `world` entries, each entry sized for the LARGEST
 *                   payload (rc_gather_bytes(RC_GATHER_FULL), rounded up to 256: rc_p2p_stride) - and flag block, and
 *                   writes an RC_P2P_EXPORT_BYTES blob; the caller hands every rank's blob to every rank (file, socket,
 *                   MPI, torch.distributed - the library does not care), rank r's at offset r * RC_P2P_EXPORT_BYTES.
 *                   Called again with another mode it only switches the payload (same buffers, same blob, sequence
 *                   numbers run on; every rank switches at the same gather);
 *   rc_p2p_connect  opens the peers' buffers (a no-op once connected);
 *   rc_gather_trajectory_p2p   sends the last step's record (the source of `mode`, see rc_gather_trajectory; the caller
 *                   double-buffers it the same way) into slot k & 1 of every rank, k = 0, 1, ... counting the calls:
 *                   queued behind the work on the handle's stream, runs on streams of its own;
 *   rc_gather_p2p_wait         orders the handle's stream (host_sync != 0: and the host) behind the COMPLETION of the LAST
 *                   issued gather - every rank's record has arrived here AND this rank's outbound copies have read their
 *                   source to the end - and returns the slot (*bytes = world x stride): rank r's record
 *                   - rc_gather_bytes(mode) bytes of it - at r * stride, stride = *bytes / world.  The slot
 *                   stays valid until the call that issues the gather after next; a peer that does not take part within
 *                   RC_P2P_TIMEOUT_S (20 s) makes the host-synchronising wait return RC_ERR_COMM instead of blocking
 *                   (reported once, the counter then starts again; the slots of that gather and the one before are not
 *                   valid on any rank - tear the transport down and set it up again).
 *                   THE RULE FOR THE SOURCE: gather k reads the record in place, asynchronously.  Call
 *                   rc_gather_p2p_wait(env, 0, ...) BEFORE issuing gather k + 1 - the handle's stream then waits for gather k,
 *                   so the step after next, which rewrites gather k's source in a double-buffered pair, runs behind it.
 *                   Without that call nothing orders a later step behind the outbound copies (records may be torn);
 *   rc_p2p_slot     the slot of the last issued gather (back = 0) or of the one before it (back = 1), without waiting;
 *   rc_p2p_disconnect          waits for this rank's copies and unmaps the peers' buffers; rc_p2p_teardown frees this rank's
 *                   own.  Exported memory must not be freed while a peer still maps it: EVERY rank disconnects, the caller
 *                   synchronises the ranks (a barrier of its own), THEN the ranks tear down (rc_destroy tears down too).
 * Every rank must issue the same sequence of gathers.  Ranks may share a GPU (functional tests) or sit on one each. */
#define RC_P2P_EXPORT_BYTES 256
int rc_p2p_setup(rc_env *env, int32_t mode, int32_t rank, int32_t world, void *export_out, size_t bytes);
int rc_p2p_connect(rc_env *env, const void *exports_world_x_256, size_t bytes);
int rc_gather_trajectory_p2p(rc_env *env);
int rc_gather_p2p_wait(rc_env *env, int32_t host_sync, void **gathered_dev, size_t *gathered_bytes);
int rc_p2p_slot(rc_env *env, int32_t back, void **gathered_dev, size_t *gathered_bytes);
int rc_p2p_disconnect(rc_env *env);
int rc_p2p_teardown(rc_env *env);

/* Re-point the output fields (everything rc_get returns except RC_F_ACTION_IN, which stays where it is) at
 * another device buffer of at least rc_arena_bytes(), 64-byte aligned; NULL = back to the handle's own arena.
 * Stream-ordered: the next rc_reset / rc_step / rc_set_pose writes there.  This is how a device-resident
 * trajectory ring is filled without copies - the step after Collect.step in the reference
 * (dreamer/wrappers.py:213-219, dreamer/tools.py:235-264): one arena per time slot, rotate before each step.
 * Lifetime: the arena a step wrote must stay allocated until the NEXT observation has been produced (small batches take
 * the cars longest-scan-first and read the previous rows for that); after rc_set_arena(env, NULL, 0) nothing of a lent
 * arena is read again, so that is the call to make before freeing one. */
int rc_set_arena(rc_env *env, void *arena, size_t bytes);

/* Rows out of a ring of arenas - the window gather of a replay sampler (the reference reads fixed-length windows out of
 * episode files: dreamer/tools.py:235-264).  ring_base + k * slot_bytes is arena k of a ring filled through rc_set_arena;
 * output row r takes the record of car car_idx[r] in slot slot_idx[r] (device int32 arrays), for every field of
 * field_mask (bit f = rc_field f): section f of the output holds n_rows records of that field back to back, sections in
 * field order, each starting on a 64-byte boundary (rc_gather_rows_bytes = the total).  Queued on the handle's stream.
 * ring_base and slot_bytes must be multiples of 64 (every slot is an arena as rc_set_arena takes it). */
size_t rc_gather_rows_bytes(rc_env *env, uint32_t field_mask, int32_t n_rows);
int rc_gather_rows(rc_env *env, const void *ring_base, size_t slot_bytes, const int32_t *slot_idx_dev, const int32_t *car_idx_dev,
                   int32_t n_rows, uint32_t field_mask, void *out_dev, size_t out_bytes);

/* Window starts for that gather, drawn on the device (the reference draws a random index into an episode file and takes
 * `length` steps from there: dreamer/tools.py:250-262).  The ring holds `count` consecutive records (`oldest` = slot of the
 * oldest, capacity slots in all); n_windows windows of `length` records of one car each, (first record, car) uniform -
 * Philox4x32-10 keyed by `seed`, counter (window, try, draw) - among the windows that stay inside one episode: no fresh record
 * strictly inside, a fresh last record only if it is the terminal transition (done).  Device int32 outputs: slot_idx /
 * slot_obs_idx / car_idx [n_windows * length] = the rows for rc_gather_rows (slot_obs_idx: a terminal row reads the slot before
 * it - for the observation fields), meta [n_windows * 4] = (ring age of the first record, car, terminal, starts an episode);
 * *failed_dev is incremented for every window that found no such start in max_tries draws.  Queued on the handle's stream. */
int rc_sample_windows(rc_env *env, const void *ring_base, size_t slot_bytes, int32_t capacity, int32_t oldest, int32_t count,
                      int32_t length, int32_t n_windows, uint64_t seed, uint32_t draw, int32_t max_tries, int32_t *slot_idx_dev,
                      int32_t *slot_obs_idx_dev, int32_t *car_idx_dev, int32_t *meta_dev, uint32_t *failed_dev);

/* One training batch in ONE call and ONE buffer: rc_sample_windows + the row gather of both kinds (observation fields
 * through slot_obs_idx, the others through slot_idx) + the reference's reset row (first row of a window that starts an episode:
 * action 0, reward 0, discount 1, time 0, progress_total -1; dreamer/wrappers.py:221-226; reset_rows = 0: records as stored).
 * Layout of out_dev (64-byte aligned): the sections of field_mask's fields in field order, each n_windows * length records,
 * each 64-byte aligned; meta int32 [n_windows][4] at *meta_offset; a 64-byte block whose first uint32 counts the windows that
 * found no episode-internal start.  Those *payload_bytes are what a sharded replay store sends (replay.ShardedReplay:
 * one collective per batch); the sampler's row indices follow as scratch, rc_sample_batch_bytes = the total to allocate.
 * A memset and two launches on the handle's stream. */
size_t rc_sample_batch_bytes(rc_env *env, uint32_t field_mask, int32_t n_windows, int32_t length, size_t *payload_bytes, size_t *meta_offset);
int rc_sample_batch(rc_env *env, const void *ring_base, size_t slot_bytes, int32_t capacity, int32_t oldest, int32_t count, int32_t length,
                    int32_t n_windows, uint64_t seed, uint32_t draw, int32_t max_tries, uint32_t field_mask, int32_t reset_rows,
                    void *out_dev, size_t out_bytes);

int rc_sync(rc_env *env);
void *rc_stream(rc_env *env);      /* the hipStream_t the handle launches on */

/* Per-kernel timing with HIP events recorded on the handle's stream.  enabled: 0 = off, 1 = every kernel,
 * otherwise a bit mask (1 << RC_K_*) of the kernels to time (fewer events in a timed region). */
int rc_set_profiling(rc_env *env, int32_t enabled);
int rc_kernel_time(rc_env *env, int32_t kernel, double *total_ms, uint64_t *launches);
int rc_reset_kernel_times(rc_env *env);

/* Raycast implementation selector, 0..7 (all variants return identical results; 7, the default, is the
 * fastest: per-cell, per-quadrant free rectangles, one wave per car; 0 is the cell-by-cell reference traversal). */
int rc_set_raycast_variant(rc_env *env, int32_t variant);
/* The symbol of the scan kernel the next rc_step launches, as rocprofv3 lists it (without namespace and argument list),
 * e.g. "rc_raycast_car_kernel<1, false, false>": template arguments = cars per env, next round prepared under the first
 * request (small batches), bounded trip loop. */
int rc_scan_kernel_name(rc_env *env, char *out, size_t bytes);

/* Experiment / validation knobs of the scan - NOT part of the product interface; every knob is 0 in production and
 * the library reads nothing from the process environment.  RAY_THREADS / RAY_SPLIT / RAY_WG_PER_CU: launch geometry
 * sweeps (tools/knob_sweep.sh); BAND_LOG2 in [-40, -10]: width of the exact-count zone of the scan as
 * max(w, h) * 2^value cells instead of 2^-21 - tests/test_gpu_parity.py narrows it to show that its corner-aimed rays
 * detect a band below the rounding bound.  Takes effect immediately (also after rc_load_track). */
enum { RC_DBG_RAY_THREADS = 0, RC_DBG_RAY_SPLIT = 1, RC_DBG_RAY_WG_PER_CU = 2, RC_DBG_BAND_LOG2 = 3,
       RC_DBG_PATCH_VARIANT = 4,    /* lidar_occupancy render experiment: bit 1 = plain instead of non-temporal stores */
       RC_DBG_SCAN_BOUNDED = 5,     /* != 0: the scan runs the build whose trip loop carries a trip budget (see below) */
       RC_DBG_SCAN_ORDER = 6,   /* 0 = production (the scan takes the cars in track order, sorted every 64 observations), 1 = car index order, k > 1 = sorted every k - 1 observations */
       RC_DBG_EXACT_CHUNK = 7,  /* k > 0: the exact render (RC_OBS_LIDAR_OCCUPANCY_REFERENCE) works on k cars at a time instead of 6 144
                                 * (at most the size its scratch was allocated for) */
    RC_DBG_COUNT = 8 };
int rc_debug_set(rc_env *env, int32_t knob, int32_t value);

/* The default scan's trip loop is unbounded in the production build (its termination is a property of the tables and
 * of the exact-count band, derived in racecar_kernels.hip; a bound costs 4 % of the scan).  The BOUNDED build of the same
 * kernel - a wave-level budget of w + h + 2 trips per round; a ray that uses it up reads "no return" - runs (a) inside
 * rc_load_track over every cell a sensor can stand in (a track whose tables make any ray overrun is refused), (b) while a
 * validation band is set, (c) under RC_DBG_SCAN_BOUNDED.  rc_scan_overruns reports how many waves of this handle's
 * bounded scans have used up a budget so far (0 unless a band was mis-set or a table is corrupt). */
int rc_scan_overruns(rc_env *env, uint64_t *count);

/* In-kernel time stamps of the default scan (analysis only, like the knobs above): when `stamps` is non-NULL the next
 * scans run an instrumented build of the one-wave-per-car kernel (1 car per env only) whose first `n_waves` waves write
 * RC_STAMP_SLOTS uint64 each to the DEVICE buffer `stamps` - shader-clock values (s_memtime) at fixed points of the wave's
 * life plus two counters; slot meanings: tools/scan_stamps.py.  NULL switches back to the production kernel. */
#define RC_STAMP_SLOTS 32
int rc_debug_scan_stamps(rc_env *env, uint64_t *stamps, int32_t n_waves);

/* Host-only: the beam (cos, sin) and footprint tables the kernels use (float32 [1080][2], [34][2]). */
void rc_spec_tables(float *beams_1080x2, float *footprint_34x2);

/* Device self-test of an arithmetic property the raycast kernel relies on: v_rcp_f32 + one FMA Newton step is
 * the correctly rounded (IEEE) reciprocal.  Checks every fp32 of both signs with biased exponent in
 * [27, 227] (2^-100 .. 2^100, 3.37e9 values) on `device`; *n_mismatch must come back 0. */
int rc_selftest_reciprocal(int32_t device, uint64_t *n_checked, uint64_t *n_mismatch);

/* The same for the square root of the reference follow-the-gap agent's arccos (ros_agent/agents/follow_the_gap/src/agent.py:171:
 * np.arccos; spec: oracle.acos32): v_sqrt_f32 alone is good to 1 ulp, the kernel's fix-up (two fused residuals) makes it the
 * correctly rounded root the spec's np.sqrt is.  Checks every positive binary32 from 2^-60 to 2^10 (587 M values) and zero
 * against the double-precision root rounded once; *n_mismatch must come back 0. */
int rc_selftest_sqrt(int32_t device, uint64_t *n_checked, uint64_t *n_mismatch);

/* The exact render (RC_OBS_LIDAR_OCCUPANCY_REFERENCE) divides the spline weights by 6 without a division instruction (a quotient
 * estimate, its exact remainder by one fused multiply-add, one correction: correctly rounded by Markstein's theorem).  This
 * compares that with the device's own binary64 division over 2^32 operands from 2^-160 to 8, either sign; n_mismatch must be 0. */
int rc_selftest_div6(int32_t device, uint64_t *n_checked, uint64_t *n_mismatch);

/* The exact render decides a pixel of the rotated window by a binary32 estimate of its 16-tap sum wherever that estimate lies more
 * than 1e-3 from a rounding boundary, and by the library's binary64 sum elsewhere (racecar_patch_exact.h, PX_BAND: the estimate's
 * error is bounded by 1.1e-4).  This renders the env's cars once more with BOTH computed for every pixel: out[0] = pixels inside
 * the array, out[1] = those the band sent to the binary64 sum, out[2] = those the estimate alone would have got wrong (0, or the
 * bound does not hold), out[3] = the largest |estimate - binary64 sum| seen, as the bits of a binary32.  The patches are written
 * as by an observation.  tests/test_gpu_api.py. */
int rc_selftest_exact_estimate(rc_env *env, uint64_t out[4]);

const char *rc_last_error(void);
int rc_abi_version(void);
/* Hash (32 hex digits) of the compiler flags and of the contents of every source and header this library was built
 * from - what racing_dreamer_amd/build.py compares with the tree beside it to decide whether to compile. */
const char *rc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* RACECAR_HIP_H */
