// reduce_kernels.hpp -- what the binned reduction (fa_reduce_*) needs beside the reducing sink of K7
// (decode_frames_kernel<..., RED = true>, decode_kernels.hpp):
//   reduce_fill_kernel    the bin arrays pre-set to the identities (INT64_MAX, INT64_MIN, 0)
//   reduce_tasks_kernel   K7's task table for a subset of streams, built on the device from the caller's stream list
//   reduce_wave_kernel    a decoded int64 column chunk folded into the bin arrays, one wave per (row, 2048-sample
//                         segment): bins of 64 samples and more
//   reduce_lane_kernel    the same with one lane per (row, bin): bins narrower than a wave
// The chunk reducers serve two-channel stores, which have no fused sink (min / max exact, the sum modulo 2^64, no
// squares).  A bin that lies wholly inside one work item's piece is written with plain stores; every other piece combines
// with 64-bit atomics -- integer min / max / add commute, so the result does not depend on the order of arrival.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

constexpr int kReduceSeg = 2048;  // samples of a row one wave of reduce_wave_kernel walks

struct ReduceOut {
    long long* mn;
    long long* mx;
    long long* sum;
    unsigned long long* sq_hi;  // null together: no squares
    unsigned long long* sq_lo;
    int64_t nbins;
};

__global__ __launch_bounds__(256) void reduce_fill_kernel(ReduceOut o, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    o.mn[i] = INT64_MAX;
    o.mx[i] = INT64_MIN;
    o.sum[i] = 0;
    if (o.sq_hi) { o.sq_hi[i] = 0; o.sq_lo[i] = 0; }
}

// task t = (row t / nfr, frame f0 + t % nfr): stream sel[row], the range [first, last), output slot row * nbins.
// A stream index outside [0, n_stream) sets `bad` in the error word and decodes stream 0 in its place.
__global__ __launch_bounds__(256) void reduce_tasks_kernel(const int64_t* __restrict__ sel, int64_t n_stream, int64_t n_tasks, int64_t nfr,
                                                           int64_t f0, int64_t first, int64_t last, int64_t nbins, int64_t* __restrict__ t_stream,
                                                           int64_t* __restrict__ t_frame, int64_t* __restrict__ t_first, int64_t* __restrict__ t_last,
                                                           int64_t* __restrict__ t_out, int* err, int bad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tasks) return;
    const int64_t row = t / nfr;
    int64_t s = sel[row];
    if (s < 0 || s >= n_stream) { atomicOr(err, bad); s = 0; }
    t_stream[t] = s;
    t_frame[t] = f0 + (t - row * nfr);
    t_first[t] = first;
    t_last[t] = last;
    t_out[t] = row * nbins;
}

struct ReduceAcc {
    long long mn = INT64_MAX, mx = INT64_MIN;
    unsigned long long sum = 0;  // (unsigned: the sum wraps modulo 2^64, as numpy's int64 sum does)
    __device__ __forceinline__ void take(long long x) {
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        sum += (unsigned long long)x;
    }
    __device__ __forceinline__ void put(const ReduceOut& o, int64_t at, bool whole) const {
        if (whole) {
            o.mn[at] = mn; o.mx[at] = mx; o.sum[at] = (long long)sum;
        } else {
            (void)__hip_atomic_fetch_min(o.mn + at, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(o.mx + at, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(o.sum + at), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

__device__ __forceinline__ unsigned long long wave_xor_u64(unsigned long long v, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// The chunk: data[row * cw + c] is sample c0 + c of row `row` (rows of the result, in order), c < cw.  The range
// [first, last) and `width` define the bins; the chunk lies inside the range.  Workgroup = one wave: workgroup b takes
// segment b % nseg (kReduceSeg samples) of row b / nseg.
__global__ __launch_bounds__(64) void reduce_wave_kernel(const long long* __restrict__ data, int64_t cw, int64_t c0, int64_t first, int64_t last,
                                                         int64_t width, int64_t nseg, ReduceOut o) {
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x / nseg;
    const int64_t p0 = c0 + ((int64_t)blockIdx.x - row * nseg) * kReduceSeg;  // this wave's piece, stream coordinates
    const int64_t p1 = (p0 + kReduceSeg < c0 + cw) ? p0 + kReduceSeg : c0 + cw;
    const long long* const src = data + row * cw;
    for (int64_t bin = (p0 - first) / width; ; ++bin) {
        const int64_t b0 = first + bin * width;
        if (b0 >= p1) break;
        const int64_t b1 = (b0 + width < last) ? b0 + width : last;
        const int64_t lo = b0 > p0 ? b0 : p0, hi = b1 < p1 ? b1 : p1;
        ReduceAcc acc;
        for (int64_t i = lo + lane; i < hi; i += 64) acc.take(src[i - c0]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long m1 = (long long)wave_xor_u64((unsigned long long)acc.mn, off);
            const long long m2 = (long long)wave_xor_u64((unsigned long long)acc.mx, off);
            acc.mn = m1 < acc.mn ? m1 : acc.mn;
            acc.mx = m2 > acc.mx ? m2 : acc.mx;
            acc.sum += wave_xor_u64(acc.sum, off);
        }
        if (lane == 0) acc.put(o, row * o.nbins + bin, lo == b0 && hi == b1);
    }
}

// One lane per (row, bin that meets the chunk): bins bin_lo .. bin_lo + n_bin - 1, nblk workgroups per row.
__global__ __launch_bounds__(256) void reduce_lane_kernel(const long long* __restrict__ data, int64_t cw, int64_t c0, int64_t first, int64_t last,
                                                          int64_t width, int64_t bin_lo, int64_t n_bin, int64_t nblk, ReduceOut o) {
    const int64_t row = (int64_t)blockIdx.x / nblk;
    const int64_t k = ((int64_t)blockIdx.x - row * nblk) * 256 + threadIdx.x;
    if (k >= n_bin) return;
    const int64_t bin = bin_lo + k;
    const int64_t b0 = first + bin * width;
    const int64_t b1 = (b0 + width < last) ? b0 + width : last;
    const int64_t lo = b0 > c0 ? b0 : c0, hi = b1 < c0 + cw ? b1 : c0 + cw;
    const long long* const src = data + row * cw;
    ReduceAcc acc;
    for (int64_t i = lo; i < hi; ++i) acc.take(src[i - c0]);
    acc.put(o, row * o.nbins + bin, lo == b0 && hi == b1);
}

}  // namespace fa
