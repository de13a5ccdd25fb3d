// find_kernels.hpp -- what the search (fa_find_*) needs beside the search sink of K7 (K7F:
// decode_frames_kernel<..., FIND = 1 | 2>, decode_kernels.hpp):
//   find_zero_kernel         the per-frame counts set to zero on the caller's stream
//   find_tasks_kernel        K7's task table for the fill pass: the frames that hold a hit, from the sorted list of
//                            their cells and the exclusive prefix sum of the counts
//   find_chunk_count_kernel  a decoded int64 column chunk counted into the same layout, one wave per (row, frame piece)
//   find_chunk_fill_kernel   the hits of such a piece written in sample order (ballot and prefix within the wave)
// The chunk kernels serve two-channel stores, which have no fused sink.
// The rule is K7F's: a sample x of row r is a hit iff (x < lo[r] || x > hi[r]) != inside.  Cell r * nfr + (f - f0) of
// frame_counts belongs to frame f of row r; every cell has exactly one writer, so plain stores do and nothing depends on
// the order of arrival.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

// What fa_find_* hand to the decode driver next to the ReduceSink that names the rows.
struct FindSink {
    const long long* lo;      // [rows]
    const long long* hi;      // [rows]
    int inside;
    int64_t n_frames;         // frames per row the caller sized its arrays with: checked against the decoder's own
    long long* frame_counts;  // count pass: [rows][n_frames]
    // fill pass (hit_ids != null)
    int64_t n_hit;
    const long long* hit_ids;  // [n_hit] cells with a non-zero count, ascending
    const long long* offs;     // [rows * n_frames + 1] exclusive prefix sum of the counts
    long long* pos;            // [total]
    long long* val;            // [total] or null
};

__global__ __launch_bounds__(256) void find_zero_kernel(long long* counts, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// task t = cell ids[t] = (row id / nfr, frame f0 + id % nfr): stream sel[row] (or row), the range [first, last), output
// base offs[id].  A cell outside [0, rows * nfr) or a stream outside [0, n_stream) sets `bad` in the error word; its task
// decodes frame f0 of stream 0 over an empty range, which writes nothing.
__global__ __launch_bounds__(256) void find_tasks_kernel(const long long* __restrict__ ids, int64_t n_tasks, int64_t rows, int64_t nfr, int64_t f0,
                                                         int64_t first, int64_t last, const int64_t* __restrict__ sel, int64_t n_stream,
                                                         const long long* __restrict__ offs, int64_t* __restrict__ t_stream,
                                                         int64_t* __restrict__ t_frame, int64_t* __restrict__ t_first, int64_t* __restrict__ t_last,
                                                         int64_t* __restrict__ t_out, int* err, int bad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tasks) return;
    const long long id = ids[t];
    bool ok = id >= 0 && id < rows * nfr;
    int64_t row = 0, s = 0;
    if (ok) {
        row = id / nfr;
        s = sel ? sel[row] : row;
        if (s < 0 || s >= n_stream) ok = false;
    }
    if (!ok) atomicOr(err, bad);
    t_stream[t] = ok ? s : 0;
    t_frame[t] = ok ? f0 + (id - row * nfr) : f0;
    t_first[t] = first;
    t_last[t] = ok ? last : first;
    t_out[t] = ok ? offs[id] : 0;
}

// The chunk: data[row * cw + c] is sample c0 + c of row `row` (rows of the result, in order), c < cw.  Workgroup = one
// wave: workgroup b takes the piece of frame fa + b % nseg (fa: the frame of sample c0) that lies in the chunk, of row
// b / nseg.  Chunks are cut at frame boundaries, so a frame's piece is all of the frame that lies in [first, last).
struct FindChunk {
    const long long* data;
    int64_t cw, c0, nseg, B, nfr, f0;
    const long long* lo;
    const long long* hi;
    int inside;
};

__device__ __forceinline__ bool find_hit(long long x, long long lo, long long hi, bool inside) { return ((x < lo) || (x > hi)) != inside; }

__global__ __launch_bounds__(64) void find_chunk_count_kernel(FindChunk c, long long* __restrict__ frame_counts) {
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x / c.nseg;
    const int64_t f = c.c0 / c.B + ((int64_t)blockIdx.x - row * c.nseg);
    const int64_t p0 = f * c.B > c.c0 ? f * c.B : c.c0;
    const int64_t p1 = (f + 1) * c.B < c.c0 + c.cw ? (f + 1) * c.B : c.c0 + c.cw;
    const long long* const src = c.data + row * c.cw;
    const long long lo = c.lo[row], hi = c.hi[row];
    const bool inside = c.inside != 0;
    uint32_t n = 0;  // (a frame holds at most 65535 samples)
    for (int64_t i = p0 + lane; i < p1; i += 64) n += find_hit(src[i - c.c0], lo, hi, inside) ? 1u : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    if (lane == 0) frame_counts[row * c.nfr + (f - c.f0)] = (long long)n;
}

// offs: the exclusive prefix sum of frame_counts (cells + 1 entries).  A wave whose cell is empty returns at once; the
// others walk their piece 64 samples at a time and place each round's hits behind the rounds before, in sample order.
__global__ __launch_bounds__(64) void find_chunk_fill_kernel(FindChunk c, const long long* __restrict__ offs, long long* __restrict__ pos,
                                                             long long* __restrict__ val) {
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x / c.nseg;
    const int64_t f = c.c0 / c.B + ((int64_t)blockIdx.x - row * c.nseg);
    const int64_t cell = row * c.nfr + (f - c.f0);
    const long long base = offs[cell];
    const long long cap = offs[cell + 1] - base;
    if (cap <= 0) return;
    const int64_t p0 = f * c.B > c.c0 ? f * c.B : c.c0;
    const int64_t p1 = (f + 1) * c.B < c.c0 + c.cw ? (f + 1) * c.B : c.c0 + c.cw;
    const long long* const src = c.data + row * c.cw;
    const long long lo = c.lo[row], hi = c.hi[row];
    const bool inside = c.inside != 0;
    long long k = 0;  // hits of the rounds so far (wave-uniform)
    for (int64_t i0 = p0; i0 < p1; i0 += 64) {
        const int64_t i = i0 + lane;
        long long x = 0;
        bool hit = false;
        if (i < p1) { x = src[i - c.c0]; hit = find_hit(x, lo, hi, inside); }
        const unsigned long long m = __ballot(hit);
        if (m == 0ull) continue;
        const long long at = k + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && at < cap) {
            pos[base + at] = i;
            if (val) val[base + at] = x;
        }
        k += __popcll(m);
    }
}

}  // namespace fa
