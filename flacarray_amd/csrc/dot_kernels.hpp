// dot_kernels.hpp -- what the inner products with templates (fa_dot_*: sum_j x[r, first + j] * T[k, j] per row and
// template) need beside their sink of K7 (K7D: decode_frames_kernel<..., DOT = KT>, decode_kernels.hpp):
//   DotSink            what the driver hands to K7D
//   dot_chunk_kernel   a decoded int64 column chunk against the template image, one wave per (row, segment)
// The chunk kernel serves two-channel stores, which have no fused sink.  K7D's task table is xsum_tasks_kernel's
// (xsum_kernels.hpp) with the trivial plan: one group, rows of 64 consecutive positions of the selection.
//
// The template image is sample-major: int32 [last - first][ld] in C order, ld >= K a multiple of 8, padding columns zero.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reduce_kernels.hpp"

namespace fa {

constexpr int kDotKT = 8;  // templates per decode of the range (K7D's pass width)

// What fa_dot_* hand to the decode driver: the trivial plan's row table, the template image and the limb arrays
// [n_sel][K] (zero-filled by the driver).  k0: the first template of this decode of the range.
struct DotSink {
    int64_t n_rows;
    const int64_t* rows;  // [n_rows][3], as XsumSink's
    int64_t K, ld, k0;
    const int32_t* tmpl;
    unsigned long long* hi;
    unsigned long long* lo;
};

// The chunk: data[row * cw + c] is sample c0 + c of result row `row`, c < cw; the chunk lies inside [first, last).
// Workgroup = one wave: workgroup b takes segment b % nseg (kReduceSeg samples) of row b / nseg and walks it once per
// template, lanes along the columns.  x = xh * 2^32 + xl with xh signed and xl unsigned; xl * t and xh * t both fit an
// int64 (|t| <= 2^31) and each is kept as a limb pair, lo += (uint32)p, hi += p >> 32 (arithmetic).  out[(row * K + k) * 4
// + 0..3] receives (hi, lo) of xl * t and (hi, lo) of xh * t:
//     dot = ((out[2] * 2^32 + out[3]) * 2^32) + (out[0] * 2^32 + out[1]),   out[0], out[2] signed, out[1], out[3] unsigned.
// A lane adds at most kReduceSeg / 64 terms below 2^32 and a cell at most last - first <= 2^32 - 1 of them: nothing wraps
// but the signed limbs, which may (two's complement).  Segments of a row and chunks of a range meet in 64-bit atomics.
__global__ __launch_bounds__(64) void dot_chunk_kernel(const long long* __restrict__ data, int64_t cw, int64_t c0, int64_t first, int64_t nseg,
                                                       const int32_t* __restrict__ tmpl, int64_t K, int64_t ld,
                                                       unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x / nseg;
    const int64_t p0 = ((int64_t)blockIdx.x - row * nseg) * kReduceSeg;  // this wave's piece, chunk coordinates
    const int64_t p1 = (p0 + kReduceSeg < cw) ? p0 + kReduceSeg : cw;
    const long long* const src = data + row * cw;
    const int32_t* const t0 = tmpl + (c0 - first) * ld;
    for (int64_t k = 0; k < K; ++k) {
        unsigned long long acc[4] = {0, 0, 0, 0};
        for (int64_t c = p0 + lane; c < p1; c += 64) {
            const long long x = src[c];
            const long long t = (long long)t0[c * ld + k];
            const long long pl = (long long)(unsigned long long)(uint32_t)x * t;
            const long long ph = (x >> 32) * t;
            acc[0] += (unsigned long long)(pl >> 32);
            acc[1] += (uint32_t)pl;
            acc[2] += (unsigned long long)(ph >> 32);
            acc[3] += (uint32_t)ph;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += wave_xor_u64(acc[j], off);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                (void)__hip_atomic_fetch_add(out + (row * K + k) * 4 + j, acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace fa
