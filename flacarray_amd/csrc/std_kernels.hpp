// std_kernels.hpp -- per-stream standard deviation with numpy's summation order (np.std(x, axis=-1)) on gfx950.
//
// S1 stream_chunk_sum_kernel<T, DEV> : one wave per (stream, chunk of `chunk` elements): the chunk's pairwise sum
//                                      (numpy's @TYPE@_pairwise_sum) of x (DEV = false) or of dtype((x - mean)^2)
//                                      (DEV = true) into the workspace
// S2 stream_fold_kernel<T, DEV>      : one thread per stream: the chunk sums added in chunk order from 0, divided by n in
//                                      double and rounded to T -> the mean (DEV = false) or sqrt of it -> the std
//
// A full chunk of 8192 elements is a perfect tree over 64 leaves of 128: lane i sums leaf i with numpy's eight strided
// accumulators, then six xor-butterfly levels add the lanes in the tree's order (IEEE addition is commutative, so both
// lanes of a pair hold the same bits).  The chunk is staged through LDS with coalesced 16-byte loads -- a lane reading
// its own 512 B leaf from HBM would touch 64 cache lines per load instruction -- in 32-unit rows padded by one 16-byte
// unit, so lane i's ds_read_b128 of unit k lands on banks 4(i + k) mod 64: no conflicts.  float64 takes two rounds of
// 64 elements per leaf through the same 33 KiB.  Every other chunk (a row's tail, rows shorter than the chunk, any other
// chunk length) follows the host's plan (flacarray_amd/npsum.py pairwise_plan): leaf sums of up to 2048 leaves at a time
// in LDS, one lane per leaf, then lane 0 runs the postfix combine program on a stack in LDS behind them (its depth is at
// most log2(chunk / 64) + 2: every leaf of a split chunk holds 64 elements or more).
// All arithmetic is explicit round-to-nearest (__fadd_rn & co.): no contraction, no reassociation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

constexpr int kStdLeaf = 128;
constexpr int kStdFastChunk = 8192;     // 64 leaves x 128: the lane-per-leaf path
constexpr int kStdLdsUnits = 64 * 33;   // 64 rows of 32 16-byte units + 1 unit of padding = 33 792 B
constexpr int kStdPlanLeaves = 2048;    // leaf sums held in LDS at a time by the plan path (16 KiB of float64)

__device__ __forceinline__ float std_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double std_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float std_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double std_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float std_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double std_mul(double a, double b) { return __dmul_rn(a, b); }

#ifndef FA_STD_MUTANT
#define FA_STD_MUTANT 0  // test-the-tests builds only (results are wrong, every access stays in bounds; profiles/std_edges.md)
#endif

// the element the pass sums: x itself, or dtype(dtype(x - mean)^2) (numpy: `x = arr - arrmean; x = x * x`)
template <typename T, bool DEV>
__device__ __forceinline__ T std_elem(T x, T mean) {
    if (!DEV) return x;
    const T d = std_sub(x, mean);
    return std_mul(d, d);
}

#if (FA_STD_MUTANT & 32)  // the deviation's square fused into the add: one rounding where numpy has two
__device__ __forceinline__ float std_fused(float r, float x, float mean) { const float d = std_sub(x, mean); return __fmaf_rn(d, d, r); }
__device__ __forceinline__ double std_fused(double r, double x, double mean) { const double d = std_sub(x, mean); return __fma_rn(d, d, r); }
#define FA_STD_ACC(r, x) (DEV ? std_fused(r, x, mean) : std_add(r, x))
#else
#define FA_STD_ACC(r, x) std_add(r, std_elem<T, DEV>(x, mean))
#endif

// numpy's pairwise_sum of one leaf (n <= 128) read element by element from global memory
template <typename T, bool DEV>
__device__ T std_leaf_global(const T* __restrict__ a, int n, T mean) {
    if (n < 8) {
#if (FA_STD_MUTANT & 64)
        T res = (T)0.0;
#else
        T res = (T)-0.0;
#endif
        for (int i = 0; i < n; ++i) res = FA_STD_ACC(res, a[i]);
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = std_elem<T, DEV>(a[j], mean);
    const int stop = n - (n % 8);
    for (int i = 8; i < stop; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = FA_STD_ACC(r[j], a[i + j]);
    }
    T res = std_add(std_add(std_add(r[0], r[1]), std_add(r[2], r[3])), std_add(std_add(r[4], r[5]), std_add(r[6], r[7])));
    for (int i = stop; i < n; ++i) res = FA_STD_ACC(res, a[i]);
    return res;
}

// Plan of one chunk length in the workspace (built by the host, std_build_plan): leaves (offset, length) as int32
// pairs, then the postfix program as bytes (1 = push the next leaf's sum, 0 = add the top two).
struct StdPlanRef {
    const int2* leaves;
    const uint8_t* ops;
    int n_leaves;
    int n_ops;
};

template <typename T, bool DEV>
FA_GLOBAL __global__ __launch_bounds__(64) void stream_chunk_sum_kernel(const T* __restrict__ in, int64_t stream_size,
                                                                       int64_t chunk, int64_t cps, const T* __restrict__ means,
                                                                       StdPlanRef plan_full, StdPlanRef plan_tail,
                                                                       T* __restrict__ chunk_sums) {
    __shared__ uint4 lds[kStdLdsUnits];
    const int lane = threadIdx.x;
    const int64_t blk = blockIdx.x;
    const int64_t s = blk / cps, c = blk - s * cps;
    const int64_t c0 = c * chunk;
    const int64_t m = (stream_size - c0 < chunk) ? stream_size - c0 : chunk;
    const T* __restrict__ a = in + s * stream_size + c0;
    const T mean = DEV ? means[s] : (T)0;
    T total;

#if (FA_STD_MUTANT & 128)  // the fast path only where the chunk itself is 8192 (the host builds no plan for a piece of 8192)
    if (m == kStdFastChunk && chunk == kStdFastChunk) {
#else
    if (m == kStdFastChunk) {
#endif
        // ---- lane-per-leaf path: ROUNDS x (64 rows of 512 B) through LDS ----
        constexpr int EPU = 16 / sizeof(T);        // elements per 16-byte unit
        constexpr int ROUNDS = sizeof(T) / 4;      // 1 (float32) or 2 (float64)
        constexpr int UPL = kStdLeaf / EPU;        // units per leaf: 32 or 64
        const bool vec = (reinterpret_cast<uintptr_t>(a) & 15) == 0;
        T r[8];
        for (int rd = 0; rd < ROUNDS; ++rd) {
            if (rd) __syncthreads();  // (the previous round's reads are done)
            if (vec) {
                const uint4* __restrict__ g = reinterpret_cast<const uint4*>(a);
                uint4 v[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) {  // unit k*64 + lane of this round: row (leaf) >> 5, unit & 31
                    const int u = k * 64 + lane;
                    v[k] = g[(u >> 5) * UPL + rd * 32 + (u & 31)];
                }
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    const int u = k * 64 + lane;
                    lds[(u >> 5) * 33 + (u & 31)] = v[k];
                }
            } else {  // unaligned row: the same image, element by element (coalesced 4- / 8-byte loads)
                T* le = reinterpret_cast<T*>(lds);
                constexpr int EPR = 32 * EPU;  // elements of one leaf per round
                for (int e = lane; e < 64 * EPR; e += 64) {
                    const int row = e / EPR, pos = e - row * EPR;
                    le[row * 33 * EPU + pos] = a[row * kStdLeaf + rd * EPR + pos];
                }
            }
            __syncthreads();
            const uint4* row = lds + lane * 33;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const uint4 u = row[k];
                T e[EPU];
                __builtin_memcpy(e, &u, 16);
#pragma unroll
                for (int q = 0; q < EPU; ++q) {
                    const int j = (k * EPU + q) & 7;  // accumulator of this element
                    if (rd == 0 && k * EPU + q < 8) r[j] = std_elem<T, DEV>(e[q], mean);  // numpy: r[j] = a[j]
                    else r[j] = FA_STD_ACC(r[j], e[q]);
                }
            }
        }
        total = std_add(std_add(std_add(r[0], r[1]), std_add(r[2], r[3])), std_add(std_add(r[4], r[5]), std_add(r[6], r[7])));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) total = std_add(total, __shfl_xor(total, off, 64));
    } else {
        // ---- plan path ----
#if (FA_STD_MUTANT & 2)
        const StdPlanRef& p = plan_tail;
#else
        const StdPlanRef& p = (m == chunk) ? plan_full : plan_tail;
#endif
        T* sums = reinterpret_cast<T*>(lds);
        T* stack = sums + kStdPlanLeaves;
        __shared__ int s_op, s_sp;
        if (lane == 0) { s_op = 0; s_sp = 0; }
        for (int base = 0; base < p.n_leaves; base += kStdPlanLeaves) {
            const int nb = (p.n_leaves - base < kStdPlanLeaves) ? p.n_leaves - base : kStdPlanLeaves;
            __syncthreads();  // (lane 0 is done with the previous batch's sums)
            for (int i = lane; i < nb; i += 64) {
                const int2 lf = p.leaves[base + i];
                sums[i] = std_leaf_global<T, DEV>(a + lf.x, lf.y, mean);
            }
            __syncthreads();
            if (lane == 0) {  // run the program up to the first push of a leaf beyond this batch
#if (FA_STD_MUTANT & 1)  // the stack pointer is not carried over a batch edge (the stack sits behind 2048 sums in LDS)
                int op = s_op, sp = 0, k = base;
#else
                int op = s_op, sp = s_sp, k = base;
#endif
                for (; op < p.n_ops; ++op) {
                    if (p.ops[op]) {
                        if (k == base + nb) break;
                        stack[sp++] = sums[k - base];
                        ++k;
                    } else {
                        const T rgt = stack[--sp];
                        stack[sp - 1] = std_add(stack[sp - 1], rgt);
                    }
                }
                s_op = op;
                s_sp = sp;
            }
        }
        __syncthreads();
        total = stack[0];
    }
    if (lane == 0) chunk_sums[blk] = total;
}

template <typename T, bool DEV>
FA_GLOBAL __global__ __launch_bounds__(256) void stream_fold_kernel(const T* __restrict__ chunk_sums, int64_t n_stream,
                                                                   int64_t stream_size, int64_t cps, T* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_stream) return;
    const T* __restrict__ cs = chunk_sums + s * cps;
#if (FA_STD_MUTANT & 64)
    T acc = (T)-0.0;
#else
    T acc = (T)0;
#endif
#if (FA_STD_MUTANT & 4)
    for (int64_t c = cps - 1; c >= 0; --c) acc = std_add(acc, cs[c]);
#else
    for (int64_t c = 0; c < cps; ++c) acc = std_add(acc, cs[c]);
#endif
#if (FA_STD_MUTANT & 8)
    const T q = sizeof(T) == 4 ? (T)__fdiv_rn((float)acc, (float)stream_size) : (T)__ddiv_rn((double)acc, (double)stream_size);
#else
    const T q = (T)__ddiv_rn((double)acc, (double)stream_size);  // numpy divides by an intp: in float64, then rounds
#endif
    // sqrt correctly rounded: hipcc lowers __fsqrt_rn to a bare v_sqrt_f32 (1 ulp), so float32 takes the float64 one (a
    // division-free Newton expansion that rounds correctly) and rounds that once more -- innocuous for a square root,
    // since 53 >= 2 * 24 + 2 bits
#if (FA_STD_MUTANT & 16)
    if (DEV) out[s] = sizeof(T) == 4 ? (T)__fsqrt_rn((float)q) : (T)__dsqrt_rn((double)q);
#else
    if (DEV) out[s] = (T)__dsqrt_rn((double)q);
#endif
    else out[s] = q;
}

}  // namespace fa
