// rc_policy_decode: the reference's LidarOccupancyDecoder (dreamer/models.py:444-465) from a feature [stoch 30 | deter 200] - a
// car's stored latent or a row of rc_policy_imagine's features - to the 64 x 64 Bernoulli logits, their mode and the count of
// pixels in which the mode differs from the car's rendered RC_F_OCCUPANCY, in the binary32 arithmetic of DESIGN.md §2 item 16
// (tests/policy_decode_spec.c is the CPU restatement): dense 230 -> 64, then four stride-2 transposed convolutions
// 1 x 1 x 64 -> 5 x 5 x 32 -> 13 x 13 x 16 -> 30 x 30 x 8 -> 64 x 64 x 1, ReLU after each.  Every output is one fmaf chain in
// the spec's order (kernel row u, kernel column v, input channel c, all ascending) from its bias.
//
// One workgroup of eight waves takes DG = 4 rows.  h1 and h2 are dense layers and run for the four rows at once (a weight is read
// once for four chains).  h3 - h5 run row by row in the GATHER form, one output parity class (y mod 2, x mod 2) at a time per wave:
// within a class every pixel has the same kernel taps u = py + 2 ty, v = px + 2 tx and reads the input pixel (Y - ty, X - tx), so
// a lane owns output pixels, the weights of a (tap, channel) are the same for the whole wave - the compiler fetches them with
// scalar loads and feeds them to v_pk_fma_f32 as SGPR pairs, two output channels (h3, h4) or two parity classes (h5) per
// instruction - and the only vector loads are the activations, one ds_read_b128 per four input channels.  Activations lie in LDS
// as planes of four channels, [c / 4][y][x][4], so that consecutive lanes (consecutive X) read consecutive 16 bytes; each map
// carries a border of two zero pixels, so that a tap that falls outside the input multiplies a zero instead of being
// predicated: fmaf(0, k, acc) = acc for the finite weights of a checkpoint (up to the sign of a zero, which the ReLU
// `acc > 0 ? acc : 0` removes).  h4 and h5 have a 6 x 6 kernel: all four classes have the same 3 x 3 taps and the same input
// pixels, so a lane computes all four (h4: a wave takes the two classes of one py) and an activation is loaded once for them.
// Intermediate activations never leave the CU.  DESIGN.md §4 has the LDS budget, the wave assignment and the issue floor.
//
// rc_policy_decode_loglik_kernel is the same body instantiated with the Bernoulli log-likelihood (DESIGN.md §2 item 22;
// tests/policy_decode_loglik_spec.c): per row the sum over the pixels of x logit - softplus(logit) against a target image x.
// Its order: a thread adds the terms of its 8 pixels (item tid, then tid + 512; in an item rows py, in a row px) from +0.0f, a
// wave adds its 64 threads in a binary tree over the lane (distance 1, 2, ..., 32), thread 0 adds the 8 waves in ascending order
// from +0.0f.  rc_policy_decode_kernel is the instantiation without it: none of this is in its code.
#include "racecar_env.h"
#include "racecar_policy_tiles.h"
#include <hip/hip_ext.h>

typedef float dc_f2 __attribute__((ext_vector_type(2)));
typedef float dc_f4 __attribute__((ext_vector_type(4)));
// A weight array as constant memory: nothing writes it while a kernel runs, and saying so is what lets the compiler fetch a
// wave-uniform address with a scalar load (the kernel's own stores would otherwise count as possible writers)
typedef const __attribute__((address_space(4))) float *dc_kptr;

namespace {

constexpr int DT = 512;                        // threads per workgroup
constexpr int DG = 4;                          // rows (images) per workgroup
constexpr int FEAT = RC_POLICY_STOCH + RC_POLICY_DETER;
constexpr int IMG = RC_POLICY_DECODE_IMAGE;
// padded maps [planes of 4 channels][side][side][4]: the input's side + 4
constexpr int S2 = 9, S3 = 17, S4 = 34;
constexpr int N_H2PAD = 8 * S2 * S2 * 4, N_H3PAD = 4 * S3 * S3 * 4, N_H4PAD = 2 * S4 * S4 * 4;      // 2592, 4624, 9248 floats
// LDS [floats]: feat [DG][230] | h1 [DG][64] | h2 [DG][800] | A = h2pad, then h4pad | B = h3pad | mismatch counter
constexpr int O_FEAT = 0, O_H1 = O_FEAT + DG * FEAT, O_H2 = O_H1 + DG * RC_DEC_H1, O_A = O_H2 + DG * RC_DEC_H2, O_B = O_A + N_H4PAD,
              O_CNT = O_B + N_H3PAD, N_LDS = O_CNT + 4;
constexpr size_t kLdsBytes = (size_t)N_LDS * sizeof(float);
constexpr size_t kLdsLoglikBytes = kLdsBytes + (DT / 64) * sizeof(float);      // the log-likelihood's eight wave sums behind the rest
static_assert(2 * kLdsLoglikBytes <= 160 * 1024, "two workgroups per CU");
static_assert(O_A % 4 == 0 && O_B % 4 == 0, "the maps are read 16 bytes at a time");

__device__ __forceinline__ float dc_relu(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ dc_kptr dc_const(const float *p) { return (dc_kptr)p; }
__device__ __forceinline__ dc_f2 dc_fma2(float a, dc_f2 w, dc_f2 acc) { return __builtin_elementwise_fma((dc_f2){a, a}, w, acc); }

// h3, one task of a wave: parity class (py, px) and output channels [4 q, 4 q + 4) of the 13 x 13 x 16 map from h2pad into h3pad
__device__ __forceinline__ void dc_h3_task(const RcDecodeDev &w, const float *A, float *B, int py, int px, int q, int lane) {
    const int ny = 7 - py, nx = 7 - px, nty = 3 - py, ntx = 3 - px;       // pixels and taps of the class
    const bool live = lane < ny * nx;
    const int item = live ? lane : 0, Y = item / nx, X = item - Y * nx;
    dc_kptr b = dc_const(w.h3_b) + 4 * q;
    dc_f2 acc0 = {b[0], b[1]}, acc1 = {b[2], b[3]};
#pragma unroll 1
    for (int ty = 0; ty < nty; ++ty) {
#pragma unroll 1
        for (int tx = 0; tx < ntx; ++tx) {
            dc_kptr k = dc_const(w.h3_k) + ((size_t)(q * 25 + (py + 2 * ty) * 5 + px + 2 * tx) * 32) * 4;      // [c][4 outputs]
            const dc_f4 *in = reinterpret_cast<const dc_f4 *>(A) + (Y - ty + 2) * S2 + (X - tx + 2);
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const dc_f4 a = in[c4 * S2 * S2];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    dc_kptr kc = k + (c4 * 4 + cc) * 4;
                    acc0 = dc_fma2(a[cc], (dc_f2){kc[0], kc[1]}, acc0);
                    acc1 = dc_fma2(a[cc], (dc_f2){kc[2], kc[3]}, acc1);
                }
            }
        }
    }
    if (live)
        reinterpret_cast<dc_f4 *>(B)[(q * S3 + 2 * Y + py + 2) * S3 + 2 * X + px + 2] =
            (dc_f4){dc_relu(acc0[0]), dc_relu(acc0[1]), dc_relu(acc1[0]), dc_relu(acc1[1])};
}

// h4: pixel block (Y, X) of the 15 x 15 blocks = lane `item`, the two classes (py, 0) and (py, 1), all 8 output channels
__device__ __forceinline__ void dc_h4(const RcDecodeDev &w, const float *B, float *A, int py, int item_in) {
    const bool live = item_in < 15 * 15;
    const int item = live ? item_in : 0, Y = item / 15, X = item - Y * 15;
    dc_f2 acc[8];                                    // [px][o / 2]
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (dc_f2){dc_const(w.h4_b)[2 * (i & 3)], dc_const(w.h4_b)[2 * (i & 3) + 1]};
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int ty = t / 3, tx = t - 3 * ty;
        dc_kptr k = dc_const(w.h4_k) + ((size_t)t * 16) * 32 + py * 16;                        // [c][py][px][8 outputs]
        const dc_f4 *in = reinterpret_cast<const dc_f4 *>(B) + (Y - ty + 2) * S3 + (X - tx + 2);
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const dc_f4 a = in[c4 * S3 * S3];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                dc_kptr kc = k + (c4 * 4 + cc) * 32;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = dc_fma2(a[cc], (dc_f2){kc[2 * i], kc[2 * i + 1]}, acc[i]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int o4 = 0; o4 < 2; ++o4) {
            const dc_f2 lo = acc[px * 4 + o4 * 2], hi = acc[px * 4 + o4 * 2 + 1];
            reinterpret_cast<dc_f4 *>(A)[(o4 * S4 + 2 * Y + py + 2) * S4 + 2 * X + px + 2] =
                (dc_f4){dc_relu(lo[0]), dc_relu(lo[1]), dc_relu(hi[0]), dc_relu(hi[1])};
        }
}

// h5: the 2 x 2 output pixels (2 Y + py, 2 X + px) of block `item` of the 32 x 32 blocks; returns them as [py][px]
__device__ __forceinline__ void dc_h5(const RcDecodeDev &w, const float *A, int item, float (&out)[4]) {
    const int Y = item >> 5, X = item & 31;
    const float b = dc_const(w.h5_b)[0];
    dc_f2 acc0 = {b, b}, acc1 = {b, b};              // py = 0, 1; each (px 0, px 1)
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int ty = t / 3, tx = t - 3 * ty;
        dc_kptr k = dc_const(w.h5_k) + (size_t)t * 8 * 4;                                      // [c][py][px]
        const dc_f4 *in = reinterpret_cast<const dc_f4 *>(A) + (Y - ty + 2) * S4 + (X - tx + 2);
#pragma unroll
        for (int c4 = 0; c4 < 2; ++c4) {
            const dc_f4 a = in[c4 * S4 * S4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                dc_kptr kc = k + (c4 * 4 + cc) * 4;
                acc0 = dc_fma2(a[cc], (dc_f2){kc[0], kc[1]}, acc0);
                acc1 = dc_fma2(a[cc], (dc_f2){kc[2], kc[3]}, acc1);
            }
        }
    }
    out[0] = dc_relu(acc0[0]); out[1] = dc_relu(acc0[1]); out[2] = dc_relu(acc1[0]); out[3] = dc_relu(acc1[1]);
}

}  // namespace

// LL: with the log-likelihood of `target` [..][64][64] (indexed as the outputs are) into `loglik` [..]
template <bool LL>
__device__ __forceinline__ void dc_decode(const RcDecodeCall &c, const uint8_t *target, float *loglik) {
    extern __shared__ float dc_lds[];
    float *feat = dc_lds + O_FEAT, *h1 = dc_lds + O_H1, *h2 = dc_lds + O_H2, *A = dc_lds + O_A, *B = dc_lds + O_B;
    int *cnt = reinterpret_cast<int *>(dc_lds + O_CNT);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * DG;
    const RcDecodeDev &w = c.w;

    // the rows' features; both maps zero: their borders stay zero from here on (only interiors are written)
    for (int idx = tid; idx < DG * FEAT; idx += DT) {
        const int g = idx / FEAT, j = idx - g * FEAT;
        const int64_t r = row0 + g;
        float v = 0.0f;
        if (r < c.n_rows) {
            if (c.features) v = c.features[(size_t)r * FEAT + j];
            else v = c.state[(size_t)pm_car(c.rows, (int)r) * RC_POLICY_STATE + j];
        }
        feat[idx] = v;
    }
    for (int idx = tid; idx < N_H4PAD + N_H3PAD; idx += DT) A[idx] = 0.0f;       // (B follows A)
    __syncthreads();

    // h1: thread (g, j) of the first 256, k ascending over stoch | deter
    if (tid < DG * RC_DEC_H1) {
        const int g = tid >> 6, j = tid & 63;
        float acc = w.h1_b[j];
#pragma unroll 10
        for (int k = 0; k < FEAT; ++k) acc = fmaf(feat[g * FEAT + k], w.h1_w[(size_t)k * RC_DEC_H1 + j], acc);
        h1[tid] = acc;
    }
    __syncthreads();
    // h2: output j = (u 5 + v) 32 + o for the four rows, c ascending; ReLU
    for (int j = tid; j < RC_DEC_H2; j += DT) {
        const float b = w.h2_b[j & 31];
        float acc[DG];
#pragma unroll
        for (int g = 0; g < DG; ++g) acc[g] = b;
#pragma unroll 8
        for (int k = 0; k < RC_DEC_H1; ++k) {
            const float kw = w.h2_k[(size_t)k * RC_DEC_H2 + j];
#pragma unroll
            for (int g = 0; g < DG; ++g) acc[g] = fmaf(h1[g * RC_DEC_H1 + k], kw, acc[g]);
        }
#pragma unroll
        for (int g = 0; g < DG; ++g) h2[g * RC_DEC_H2 + j] = dc_relu(acc[g]);
    }
    __syncthreads();

#pragma unroll 1
    for (int g = 0; g < DG; ++g) {
        const int64_t r = row0 + g;
        if (r >= c.n_rows) break;                                                  // (the same for every thread)
        const size_t at = c.features ? (size_t)r : (size_t)pm_car(c.rows, (int)r);       // the row of the outputs
        // h2pad: the whole of it, border zero (h4pad of the previous row lay here)
        for (int idx = tid; idx < N_H2PAD; idx += DT) {
            const int ci = idx & 3, p = idx >> 2, x = p % S2, y = (p / S2) % S2, c4 = p / (S2 * S2);
            const bool inside = x >= 2 && x < 7 && y >= 2 && y < 7;
            A[idx] = inside ? h2[g * RC_DEC_H2 + ((y - 2) * 5 + (x - 2)) * 32 + c4 * 4 + ci] : 0.0f;
        }
        if (tid == 0) *cnt = 0;
        __syncthreads();
        // h3: 16 tasks (class, quarter of the channels) of 9, 6, 6 and 4 taps; a wave takes two that add up to 13 or 12
        {
            const int q = wave & 3, second = wave >> 2;
            dc_h3_task(w, A, B, 0, second, q, lane);
            dc_h3_task(w, A, B, 1, 1 - second, q, lane);
        }
        __syncthreads();
        // what h2pad left where h4pad's border lies (h4pad's border beyond it is zero already; its interior is written below)
        for (int idx = tid; idx < N_H2PAD; idx += DT) {
            const int p = idx >> 2, x = p % S4, y = p / S4;                        // (plane 0: N_H2PAD < S4 S4 4)
            if (x < 2 || x >= 32 || y < 2 || y >= 32) A[idx] = 0.0f;
        }
        dc_h4(w, B, A, wave & 1, (wave >> 1) * 64 + lane);
        __syncthreads();
        // h5 and the outputs: two blocks of 2 x 2 pixels per thread
        int differ = 0;
        float ll = 0.0f;
#pragma unroll 1
        for (int i = 0; i < 2; ++i) {
            const int item = tid + DT * i, Y = item >> 5, X = item & 31;
            float v[4];
            dc_h5(w, A, item, v);
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                const size_t p = at * (IMG * IMG) + (size_t)(2 * Y + py) * IMG + 2 * X;
                const float v0 = v[2 * py], v1 = v[2 * py + 1];
                const uint32_t bits = (v0 > 0.0f ? 1u : 0u) | (v1 > 0.0f ? 0x100u : 0u);
                if (c.logits) *reinterpret_cast<dc_f2 *>(c.logits + p) = (dc_f2){v0, v1};
                if (c.image) *reinterpret_cast<uint16_t *>(c.image + p) = (uint16_t)bits;
                if (c.mismatch) differ += __popc(bits ^ (uint32_t)*reinterpret_cast<const uint16_t *>(c.occupancy + p));
                if constexpr (LL) {
                    if (loglik) {
                        const uint32_t x = *reinterpret_cast<const uint16_t *>(target + p);
                        ll = ll + (((x & 0xffu) ? v0 : 0.0f) - pm_softplus(v0));
                        ll = ll + (((x >> 8) ? v1 : 0.0f) - pm_softplus(v1));
                    }
                }
            }
        }
        if constexpr (LL) {
            if (loglik) {                                                          // (the same for every thread)
                float *wsum = dc_lds + N_LDS;
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) ll = ll + __shfl_xor(ll, m, 64);
                if (lane == 0) wsum[wave] = ll;
                __syncthreads();
                if (tid == 0) {
                    float sum = 0.0f;
#pragma unroll
                    for (int k = 0; k < DT / 64; ++k) sum = sum + wsum[k];
                    loglik[at] = sum;
                }
            }
        }
        if (c.mismatch) {
            if (differ) atomicAdd(cnt, differ);
            __syncthreads();
            if (tid == 0) c.mismatch[at] = *cnt;
        }
        __syncthreads();                                                           // the next row's h2pad overwrites h4pad
    }
}

__global__ __launch_bounds__(DT) void rc_policy_decode_kernel(RcDecodeCall c) { dc_decode<false>(c, nullptr, nullptr); }

__global__ __launch_bounds__(DT) void rc_policy_decode_loglik_kernel(RcDecodeLoglikCall c) { dc_decode<true>(c.d, c.target, c.loglik); }

hipError_t rck_decode_prepare() {
    const hipError_t e = hipFuncSetAttribute((const void *)rc_policy_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)rc_policy_decode_loglik_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLoglikBytes);
}

hipError_t rck_launch_decode(const RcDecodeCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.n_rows + DG - 1) / DG);
    hipExtLaunchKernelGGL(rc_policy_decode_kernel, dim3(blocks), dim3(DT), (uint32_t)kLdsBytes, s, start, stop, 0u, c);
    return hipGetLastError();
}

hipError_t rck_launch_decode_loglik(const RcDecodeLoglikCall &c, hipEvent_t start, hipEvent_t stop, hipStream_t s) {
    const unsigned blocks = (unsigned)((c.d.n_rows + DG - 1) / DG);
    hipExtLaunchKernelGGL(rc_policy_decode_loglik_kernel, dim3(blocks), dim3(DT), (uint32_t)kLdsLoglikBytes, s, start, stop, 0u, c);
    return hipGetLastError();
}
