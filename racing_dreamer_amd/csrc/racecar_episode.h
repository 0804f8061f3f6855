// The episode log on the device (racecar_episode.hip): what the C-ABI layer and the kernels share.
// Not part of the public interface (the row and the counters are: include/racecar_hip.h, rc_episode_row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RC_EP_BLOCK 256                          // envs per workgroup of the three kernels (one env per lane)
enum { RC_EPC_WRITTEN = 0, RC_EPC_DROPPED = 1, RC_EPC_SKIPPED = 2, RC_EPC_ABANDONED = 3, RC_EPC_AT_QUOTA = 4, RC_EPC_CALLS = 5,
       RC_EPC_COUNT = 6 };

struct RcEpisodeRow {                            // = rc_episode_row, 48 bytes
    int32_t env, slot, track;
    uint32_t episode, call;
    int32_t length;
    float ret, progress, time;
    int32_t laps;
    uint32_t flags, reserved;
};

struct RcEpisodeDev {
    // what the step (or the reset) left in the output arena, [n_cars] each (the CURRENT arena: rc_set_arena re-points them)
    const float *reward, *progress_total, *time;
    const int32_t *lap;
    const uint8_t *done, *trunc, *wall, *opp, *wrong, *fresh;
    const int32_t *ts_track;                     // [num_envs] the env's current track, or null without a track set
    int32_t ts_n;
    // the running episode, handle-owned: per env ...
    uint8_t *active;                             // 1 while an episode that started at a reset seen by the log is running
    uint32_t *ordinal;                           // episodes of this env that ended since enable / clear
    int32_t *length, *track;                     // calls so far; the track latched at the episode's start
    // ... and per car
    float *ret, *prog_max, *time_max;
    uint8_t *wrong_seen;
    // the log
    RcEpisodeRow *rows;
    unsigned long long capacity;                 // rows
    uint32_t max_episodes;                       // per-env quota, 0 = none
    unsigned long long *counters;                // [RC_EPC_COUNT]
    unsigned long long *cursor;                  // [2] rows asked for so far (written + dropped), by call parity
    uint32_t *block_counts;                      // [blocks] envs of the workgroup that put rows into the log in this call
    int32_t num_envs, cars_per_env;
    uint32_t first_env, call;
};

// A step: count (per workgroup, the envs that log in this call), then update (sums, rows at cursor + the exclusive prefix
// of the counts, re-arm).  Both on `s`, after the dynamics launch.
hipError_t rck_launch_episode_step(const RcEpisodeDev &d, hipStream_t s);
// rc_reset: the envs of the mask (null = all) abandon a running episode and start one.  After the reset launch.
hipError_t rck_launch_episode_reset(const RcEpisodeDev &d, const uint8_t *mask_dev, hipStream_t s);
