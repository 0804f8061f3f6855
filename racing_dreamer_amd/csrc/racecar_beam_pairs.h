// The beam table's second image (RcTrackDev::beam_pairs): the one-wave-per-car scan reads the (cos, sin) pairs of TWO rounds with
// one 16-byte load per lane.  Plain C++, no device code: rc_load_track builds the image with it, and a stand-alone program
// (tests/beam_pairs_check.cpp) checks that it is a re-arrangement of the per-round table and nothing else.
#pragma once
#include <stddef.h>
#include <string.h>

#define RC_BEAM_ROUNDS 17                                  // 1080 beams in rounds of 64 lanes, the last one partial
#define RC_BEAM_PAIR_RECORDS ((RC_BEAM_ROUNDS + 1) / 2)     // 9 records of 64 lanes x 16 bytes

// per_round: [RC_BEAM_ROUNDS * 64][2] floats, beam 64 r + lane at entry 64 r + lane (the padded table of rc_load_track).
// paired:    [RC_BEAM_PAIR_RECORDS * 64][4] floats, entry 64 k + lane = the pairs of beams 128 k + lane (round 2 k) and
//            128 k + 64 + lane (round 2 k + 1).  There is no round 17: the last record's second half is zeros, like the per-round
//            table's own padding behind beam 1079, and no round reads it.
// The words are copied as they are (memcpy: no conversion that could touch a bit).
static inline void rc_pair_beams(const float *per_round, float *paired) {
    for (int k = 0; k < RC_BEAM_PAIR_RECORDS; ++k)
        for (int lane = 0; lane < 64; ++lane) {
            float *dst = paired + ((size_t)64 * k + lane) * 4;
            memcpy(dst, per_round + ((size_t)128 * k + lane) * 2, 8);
            if (2 * k + 1 < RC_BEAM_ROUNDS)
                memcpy(dst + 2, per_round + ((size_t)128 * k + 64 + lane) * 2, 8);
            else
                memset(dst + 2, 0, 8);
        }
}
