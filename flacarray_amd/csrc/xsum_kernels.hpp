// xsum_kernels.hpp -- what the fold across streams (fa_xsum_*: per-sample sums over groups of streams) needs beside its
// sink of K7 (K7X: decode_frames_kernel<..., XSUM = true>, decode_kernels.hpp):
//   xsum_tasks_kernel   K7's task table in the layout K7X folds: a wave holds ONE frame of the 64 streams of one plan row
//   xsum_chunk_kernel   a decoded int64 column chunk summed per (group, column), one lane each
// The chunk kernel serves two-channel stores, which have no fused sink (the sum modulo 2^64, no squares).
//
// The plan is made on the host (flacarray_amd/libflacarray.py, xsum_plan): the selected streams stable-sorted by their
// group label (`order`, n_sel stream indices) and a row table of three int64 per row -- [group, first position in
// `order`, real lanes (1..64)] -- with one row per 64 lanes of one group.  Rows of a group are adjacent.  Both arrays are
// device memory the caller filled, so every entry is checked here before it becomes an address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

// What fa_xsum_* hand to the decode driver: the plan and the result arrays [n_groups][last - first] (zero-filled by the
// driver; sq_hi / sq_lo null together: no squares).
struct XsumSink {
    int64_t n_rows;
    const int64_t* rows;  // [n_rows][3]
    int64_t n_groups;
    long long* sum;
    unsigned long long* sq_hi;
    unsigned long long* sq_lo;
};

// a row of the plan, checked: false where it names a group, a position or a lane count outside the arrays
__device__ __forceinline__ bool xsum_row(const int64_t* __restrict__ rows, int64_t row, int64_t n_sel, int64_t n_groups, int64_t& group,
                                         int64_t& pos0, int64_t& real) {
    group = rows[3 * row]; pos0 = rows[3 * row + 1]; real = rows[3 * row + 2];
    return group >= 0 && group < n_groups && real >= 1 && real <= 64 && pos0 >= 0 && pos0 <= n_sel - real;
}

// task t = (wave t / 64, lane t % 64); wave w = row * nfr + fi holds frame f0 + fi of the streams order[pos0 .. pos0 + real)
// of plan row `row`, lane = position within the row.  The output offset group * n makes K7's row0 = out_off + (fstart -
// first) the index of the frame's sample 0 in the group's row of the result.  A padding lane (lane >= real) decodes the
// row's first stream over an empty range: it is never folded.  A row that fails its checks or a stream outside
// [0, n_stream) sets `bad` in the error word and becomes padding (of stream 0).
__global__ __launch_bounds__(256) void xsum_tasks_kernel(const int64_t* __restrict__ order, int64_t n_sel, const int64_t* __restrict__ rows,
                                                         int64_t n_rows, int64_t n_groups, int64_t n_stream, int64_t nfr, int64_t f0,
                                                         int64_t first, int64_t last, int64_t* __restrict__ t_stream,
                                                         int64_t* __restrict__ t_frame, int64_t* __restrict__ t_first, int64_t* __restrict__ t_last,
                                                         int64_t* __restrict__ t_out, int* err, int bad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_rows * nfr * 64) return;
    const int64_t w = t >> 6, lane = t & 63;
    const int64_t row = w / nfr, fi = w - row * nfr;
    int64_t group, pos0, real;
    bool ok = xsum_row(rows, row, n_sel, n_groups, group, pos0, real);
    int64_t s = 0;
    if (ok) {
        s = order[pos0 + (lane < real ? lane : 0)];
        if (s < 0 || s >= n_stream) { ok = false; s = 0; }
    }
    if (!ok) atomicOr(err, bad);
#if defined(FA_XSUM_MUTANT) && (FA_XSUM_MUTANT & 8)
    const bool live = ok;
#else
    const bool live = ok && lane < real;
#endif
    t_stream[t] = s;
    t_frame[t] = f0 + fi;
    t_first[t] = first;
    t_last[t] = live ? last : first;
    t_out[t] = ok ? group * (last - first) : 0;
}

// The chunk: data[p * cw + c] is sample c0 + c of stream order[p] (the rows of the chunk are the sorted selection), c < cw.
// Lane (g, c) walks the plan rows of group g and stores the sum of their streams' samples modulo 2^64 to
// sum[g * n + (c0 - first) + c]: every cell has one owner, so plain stores do.  A group without rows stores 0.
__global__ __launch_bounds__(256) void xsum_chunk_kernel(const long long* __restrict__ data, int64_t cw, int64_t c0, int64_t first, int64_t n,
                                                         int64_t n_sel, const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_groups,
                                                         long long* __restrict__ sum) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cw) return;
    for (int64_t g = blockIdx.y; g < n_groups; g += gridDim.y) {  // (grid-stride: more groups than a grid's y extent)
        unsigned long long acc = 0;  // (unsigned: the sum wraps modulo 2^64, as numpy's int64 sum does)
        for (int64_t r = 0; r < n_rows; ++r) {
            int64_t group, pos0, real;
            if (!xsum_row(rows, r, n_sel, n_groups, group, pos0, real) || group != g) continue;
            for (int64_t k = 0; k < real; ++k) acc += (unsigned long long)data[(pos0 + k) * cw + c];
        }
        sum[g * n + (c0 - first) + c] = (long long)acc;
    }
}

}  // namespace fa
