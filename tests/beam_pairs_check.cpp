// Stand-alone check of rc_pair_beams (racing_dreamer_amd/csrc/racecar_beam_pairs.h): the beam table's paired image is a pure
// re-arrangement of the per-round table - every word equal, every word of the per-round table placed exactly once, the rest
// zeros, nothing written behind the image.  Built and run by tests/test_beam_pairs.py; no GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "racecar_beam_pairs.h"

static int check(const std::vector<uint32_t> &words, const char *what) {
    const size_t n_round = (size_t)RC_BEAM_ROUNDS * 64 * 2, n_pair = (size_t)RC_BEAM_PAIR_RECORDS * 64 * 4, guard = 64;
    if (words.size() != n_round) return 1;
    std::vector<float> per_round(n_round), paired(n_pair + guard);
    std::memcpy(per_round.data(), words.data(), n_round * 4);
    const uint32_t canary = 0xA5A5A5A5u;
    for (size_t i = 0; i < n_pair + guard; ++i) std::memcpy(&paired[i], &canary, 4);
    rc_pair_beams(per_round.data(), paired.data());
    std::vector<uint32_t> got(n_pair + guard);
    std::memcpy(got.data(), paired.data(), got.size() * 4);
    int bad = 0;
    std::vector<int> placed(n_round, 0);
    for (int k = 0; k < RC_BEAM_PAIR_RECORDS; ++k)
        for (int lane = 0; lane < 64; ++lane)
            for (int half = 0; half < 2; ++half)
                for (int c = 0; c < 2; ++c) {
                    const int round = 2 * k + half;
                    const uint32_t g = got[((size_t)64 * k + lane) * 4 + 2 * half + c];
                    if (round < RC_BEAM_ROUNDS) {
                        const size_t src = ((size_t)64 * round + lane) * 2 + c;      // what the per-round load of that round reads
                        bad += g != words[src];
                        placed[src] += 1;
                    } else {
                        bad += g != 0u;                                              // "round 17": zeros
                    }
                }
    for (size_t i = 0; i < n_round; ++i) bad += placed[i] != 1;
    for (size_t i = n_pair; i < n_pair + guard; ++i) bad += got[i] != canary;
    std::printf("beam_pairs_check %s: %zu words in, %zu words out, %d wrong\n", what, n_round, n_pair, bad);
    return bad;
}

int main() {
    const size_t n_round = (size_t)RC_BEAM_ROUNDS * 64 * 2;
    // (a) the table as it is: cos / sin of 1080 beams over 270 degrees, zero padding behind beam 1079
    std::vector<uint32_t> a(n_round, 0u);
    for (int i = 0; i < 1080; ++i) {
        const double half = 135.0 * 3.14159265358979323846 / 180.0, ang = half - (double)i * (2.0 * half / 1079.0);
        const float cs[2] = {(float)std::cos(ang), (float)std::sin(ang)};
        std::memcpy(&a[2 * (size_t)i], cs, 8);
    }
    // (b) every word different, patterns that are NaNs, denormals and negative zeros as floats among them: a copy through a
    // float conversion would not survive these
    std::vector<uint32_t> b(n_round);
    for (size_t i = 0; i < n_round; ++i) b[i] = (uint32_t)i * 0x9E3779B9u + 0x7FC00001u;
    b[1] = 0x80000000u; b[2] = 0x00000001u; b[3] = 0x7F800001u; b[n_round - 1] = 0xFFFFFFFFu;
    const int bad = check(a, "beams") + check(b, "patterns");
    return bad == 0 ? 0 : 1;
}
