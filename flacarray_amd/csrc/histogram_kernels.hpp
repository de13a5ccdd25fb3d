// histogram_kernels.hpp -- what the value histogram (fa_histogram_*) needs beside the histogram sink of K7
// (decode_frames_kernel<..., HIST = true>, decode_kernels.hpp):
//   hist_fill_kernel   counts / below / above set to zero on the caller's stream
//   hist_wave_kernel   a decoded int64 column chunk counted into the same arrays, one wave per (row, 2048-sample
//                      segment), for two-channel stores, which have no fused sink
// The bin rule is K7H's: a sample x of row r below lo[r] counts in below[r]; otherwise its bin is
// ((uint64)x - (uint64)lo[r]) >> shift[r] -- the unsigned difference is exact for any x >= lo, INT64_MAX - INT64_MIN
// included -- counted in counts[r * nbins + bin] or, from nbins on, in above[r].  Everything is flushed with 64-bit
// atomics, so a bin that several chunks meet comes out right.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reduce_kernels.hpp"

namespace fa {

struct HistOut {
    unsigned long long* counts;  // [rows][nbins]
    unsigned long long* below;   // [rows]
    unsigned long long* above;   // [rows]
    const long long* lo;         // [rows]
    const int32_t* shift;        // [rows], 0..63
    int64_t nbins;               // 1..kHistMaxBins
};

__global__ __launch_bounds__(256) void hist_fill_kernel(HistOut o, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows * o.nbins) o.counts[i] = 0;
    if (i < rows) { o.below[i] = 0; o.above[i] = 0; }
}

// The chunk: data[row * cw + c] is sample c of the chunk of row `row` (rows of the result, in order), c < cw.
// Workgroup = one wave: workgroup b takes segment b % nseg (kReduceSeg samples) of row b / nseg.
__global__ __launch_bounds__(64) void hist_wave_kernel(const long long* __restrict__ data, int64_t cw, int64_t nseg, HistOut o) {
    __shared__ uint32_t hist[2048];  // (a wave counts kReduceSeg samples: uint32 is enough)
    static_assert(kReduceSeg <= 0x7fffffff, "segment counts fit uint32");
    const int lane = threadIdx.x;
    const uint32_t nb = (uint32_t)o.nbins;
    const int64_t row = (int64_t)blockIdx.x / nseg;
    const int64_t p0 = ((int64_t)blockIdx.x - row * nseg) * kReduceSeg;
    const int64_t p1 = (p0 + kReduceSeg < cw) ? p0 + kReduceSeg : cw;
    const long long* const src = data + row * cw;
    const long long lo = o.lo[row];
    const uint32_t sh = (uint32_t)o.shift[row] & 63u;
    for (uint32_t b = (uint32_t)lane; b < nb; b += 64) hist[b] = 0u;
    __syncthreads();
    uint32_t bel = 0, abv = 0;
    for (int64_t i = p0 + lane; i < p1; i += 64) {
        const long long x = src[i];
        if (x < lo) {
            bel++;
        } else {
            const unsigned long long b = ((unsigned long long)x - (unsigned long long)lo) >> sh;
            if (b >= (unsigned long long)nb) abv++;
            else (void)atomicAdd(hist + (uint32_t)b, 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = (uint32_t)lane; b < nb; b += 64) {
        const uint32_t c = hist[b];
        if (c) (void)__hip_atomic_fetch_add(o.counts + row * o.nbins + b, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        bel += (uint32_t)__shfl_xor((int)bel, off, 64);
        abv += (uint32_t)__shfl_xor((int)abv, off, 64);
    }
    if (lane == 0) {
        if (bel) (void)__hip_atomic_fetch_add(o.below + row, (unsigned long long)bel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (abv) (void)__hip_atomic_fetch_add(o.above + row, (unsigned long long)abv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace fa
