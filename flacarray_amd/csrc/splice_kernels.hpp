// splice_kernels.hpp -- K10, FlacArray.append and FlacArray.overwrite on gfx950: replace a frame-aligned span of some or all
// streams of a store by a fresh encode of it, without re-encoding the rest of the store.
//
// A frame is analysed from its own samples only.  So new samples in [first, first + n) change the frames f0 .. f1 - 1 that
// overlap the range (f0 = first / B, f1 = min(F, ceil((first + n) / B))) and no other; the span [f0 B, min(f1 B, N))
// starts on a frame boundary and ends on one or at the end of the stream, so a one-shot encode of the patched span image
// IS those frames, numbered from 0.  Likewise the frames of concat(a, b) are the frames of a followed by the frames of
// (tail of a) + b: appending is the splice whose span is the old short last frame (f0 = the old full frames, f1 = F, an
// empty span when the old stream ends on a frame boundary), whose image is that tail followed by the new samples, and
// whose encode has more frames than the span had.  With nfe the frames of the encode, the result has
// nf_new = f0 + nfe + (F - f1) frames and is, per participating stream,
//     [ 46 header bytes of size_new and nf_new, MD5 zero ][ seek points < f0 ][ nfe new points ][ points >= f1, offset + delta ]
//     [ frames < f0, verbatim ][ nfe new frames, renumbered k -> f0 + k ][ frames >= f1, verbatim, moved by delta ]
// with delta = new_mid - old_mid the change in the bytes of the middle frames; a stream that does not take part is copied
// whole.  The frames behind the span keep their numbers, which needs an empty suffix (f1 == F: append) or an unchanged
// frame count (nfe == f1 - f0: overwrite); the host's plan refuses anything else.
//
// Renumbering changes a frame's UTF-8 number field (its length may grow), its header CRC-8 and its CRC-16; the CRC-16 is
// linear (poly 0x8005, zero init, no final xor):
//     crc(H || P) = crc(H) * x^(8|P|) + crc(P)  mod G,  so  crc_new = crc_old ^ (crc(H_old) ^ crc(H_new)) * x^(8|P|) mod G
// -- O(log |P|) work per frame, no pass over its payload.  All streams share their frame numbers, so the growth of the
// number fields is one constant for every stream (append_growth), and each stream's new size is a sum of sizes the
// device already holds (splice_size_kernel).  The copy is one launch (splice_kernel): 16-byte destination chunks, each
// assembled from two aligned 16-byte source loads by a byte funnel shift (the source/destination misalignment of a
// segment is one value for all its chunks), plain vector stores; only the edges of a segment and the few computed header
// bytes are stored byte by byte.
//
// K10a splice_check_kernel  one thread per participating stream: index in range and not named twice, the layout checks of
//                           old_stream_kept, the seek offsets of f0 and f1 ordered and inside the body; gathers the
//                           participating streams' (start, nbytes) for the span decode.  Runs before anything is decoded.
// K10b splice_size_kernel   one thread per stream: the new size, and off_old(f0) / off_old(f1) for the splice.
// K10c splice_kernel        one launch, `parts` workgroups per stream (~64 KB of output each), no dependencies between
//                           workgroups, plain vector and byte stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_kernels.hpp"  // (load_be64)
#include "encode_placed.hpp"

namespace fa {

// ---- CRC-16 arithmetic in GF(2)[x] / G, G = x^16 + x^15 + x^2 + 1 ---------------------------------------
FA_HD uint32_t crc16_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 16; ++i)
        if ((b >> i) & 1u) p ^= a << i;
    for (int i = 31; i >= 16; --i)
        if ((p >> i) & 1u) p ^= 0x18005u << (i - 16);
    return p;
}
// x^(8 n) mod G by square-and-multiply
FA_HD uint32_t crc16_xpow8(uint64_t n) {
    uint32_t r = 1, b = 0x100;  // x^8
    while (n) {
        if (n & 1) r = crc16_mulmod(r, b);
        b = crc16_mulmod(b, b);
        n >>= 1;
    }
    return r;
}

// bytes of FLAC's UTF-8 coding of v (RFC 9639 9.1.5) and their sum over [0, m): sum_t max(0, m - t) over the thresholds
FA_HD int utf8_bytes(uint64_t v) {
    return v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : v < 0x80000000ULL ? 6 : 7;
}
FA_HD int64_t utf8_bytes_above(int64_t m, int64_t t) { return (m > t) ? m - t : 0; }
FA_HD int64_t utf8_bytes_below(int64_t m) {
    return utf8_bytes_above(m, 0) + utf8_bytes_above(m, 0x80) + utf8_bytes_above(m, 0x800) + utf8_bytes_above(m, 0x10000) +
           utf8_bytes_above(m, 0x200000) + utf8_bytes_above(m, 0x4000000) + utf8_bytes_above(m, 0x80000000LL);
}
// extra header bytes of frames [0, k) of the new encode once renumbered to [base, base + k)
FA_HD int64_t append_growth(int64_t base, int64_t k) { return utf8_bytes_below(base + k) - utf8_bytes_below(base) - utf8_bytes_below(k); }

struct SpliceArgs {
    const uint8_t* old;  // the old store
    int64_t old_bytes;
    const int64_t* old_starts;
    const int64_t* old_nbytes;
    const int64_t* sidx;  // [m] flat stream indices of the participating streams; NULL: all streams, in order
    int32_t* slot;        // [n_stream] row of a stream in the span encode, -1: does not take part (unused when sidx is NULL)
    int64_t* sub_starts;  // [m] the participating streams' starts and sizes (the span decode's index)
    int64_t* sub_nbytes;
    const uint8_t* enc;  // the encode of the patched span image, m streams
    int64_t enc_bytes;
    const int64_t* enc_starts;
    const int64_t* enc_nbytes;
    int64_t* off0;  // [n_stream] bytes of the frames < f0 and < f1 of a participating old stream (written by the size kernel)
    int64_t* off1;
    const int64_t* starts;  // the new store
    int64_t* nbytes;
    uint8_t* out;
    int* err;  // 2: a stream's layout, 4: the stream index
    int64_t n_stream, m, size_old, size_new, f0, f1, nf_old, nf_new;
    int32_t B, nch, parts;
};

// frames of the fresh encode: nf_new = f0 + nfe + (nf_old - f1)
__device__ __forceinline__ int64_t splice_nfe(const SpliceArgs& a) { return a.nf_new - a.f0 - (a.nf_old - a.f1); }

// The old stream must be one this encoder wrote for THIS call: "fLaC", STREAMINFO first and not last with block size B,
// the call's channel count and the call's stream size (the 36-bit total), the SEEKTABLE last with one point per frame.
// Returns false otherwise; *kept = the bytes of its frames < `frame` (the body's end stands in for frame nf_old).
__device__ __forceinline__ bool old_stream_kept(const SpliceArgs& a, int64_t s, int64_t frame, int64_t* kept) {
    const int64_t hb_old = stream_header_bytes(a.nf_old);
    const int64_t os = a.old_starts[s], on = a.old_nbytes[s];
    *kept = 0;
    if (os < 0 || on < hb_old || os + on > a.old_bytes) return false;
    const uint8_t* h = a.old + os;
    const uint32_t stl = ((uint32_t)h[43] << 16) | ((uint32_t)h[44] << 8) | h[45];
    const uint64_t packed = load_be64(h + 18);  // rate 20 | channels - 1: 3 | bits - 1: 5 | total samples: 36
    const uint64_t total = ((uint64_t)a.size_old < (1ULL << 36)) ? (uint64_t)a.size_old : 0;
    if (h[0] != 'f' || h[1] != 'L' || h[2] != 'a' || h[3] != 'C' || h[4] != 0 || h[42] != 0x83 || stl != 18u * (uint32_t)a.nf_old ||
        h[8] != (uint8_t)(a.B >> 8) || h[9] != (uint8_t)a.B || (int)((packed >> 41) & 7u) + 1 != a.nch ||
        (packed & ((1ULL << 36) - 1)) != total)
        return false;
    const int64_t k = (frame < a.nf_old) ? (int64_t)load_be64(h + 46 + 18 * frame + 8) : on - hb_old;
    if (k < 0 || k > on - hb_old) return false;
    *kept = k;
    return true;
}

// off_old(f0) and off_old(f1) of old stream s after the layout checks: both inside the body and ordered, or false.
__device__ __forceinline__ bool splice_bounds(const SpliceArgs& a, int64_t s, int64_t* o0, int64_t* o1) {
    const bool ok0 = old_stream_kept(a, s, a.f0, o0);
    const bool ok1 = old_stream_kept(a, s, a.f1, o1);
    return ok0 && ok1 && *o0 <= *o1;
}

__device__ __forceinline__ int64_t splice_row(const SpliceArgs& a, int64_t s) { return a.sidx ? (int64_t)a.slot[s] : s; }

// ---- K10a (slot is all -1 before the launch) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void splice_check_kernel(SpliceArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    int64_t s = j;
    a.sub_starts[j] = 0;
    a.sub_nbytes[j] = 0;
    if (a.sidx) {
        s = a.sidx[j];
        if (s < 0 || s >= a.n_stream || atomicExch(&a.slot[s], (int32_t)j) != -1) {
            atomicOr(a.err, 4);
            return;
        }
    }
    int64_t o0, o1;
    if (!splice_bounds(a, s, &o0, &o1)) {
        atomicOr(a.err, 2);
        return;
    }
    a.sub_starts[j] = a.old_starts[s];
    a.sub_nbytes[j] = a.old_nbytes[s];
}

// ---- K10b -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void splice_size_kernel(SpliceArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_stream) return;
    const int64_t os = a.old_starts[s], on = a.old_nbytes[s];
    const int64_t j = splice_row(a, s);
    int64_t o0 = 0, o1 = 0, size = on;
    if (j < 0) {  // copied whole: the copy reads [os, os + on)
        if (os < 0 || on < 0 || os + on > a.old_bytes) {
            atomicOr(a.err, 2);
            size = 0;
        }
    } else {
        const int64_t nfe = splice_nfe(a);
        const int64_t hb_enc = stream_header_bytes(nfe);
        const int64_t es = a.enc_starts[j], en = a.enc_nbytes[j];
        if (!splice_bounds(a, s, &o0, &o1) || es < 0 || en < hb_enc || es + en > a.enc_bytes) {
            atomicOr(a.err, 2);
            o0 = o1 = 0;
            size = 0;
        } else {
            size = on + (stream_header_bytes(a.nf_new) - stream_header_bytes(a.nf_old)) - (o1 - o0) + (en - hb_enc) + append_growth(a.f0, nfe);
        }
    }
    a.off0[s] = o0;
    a.off1[s] = o1;
    a.nbytes[s] = size;
}

// ---- K10c: the copy ---------------------------------------------------------------------------------------------------
// Copy [src, src + len) to [dst, dst + len): the 16-byte destination chunks that meet the range are shared out over
// `nthr` threads (this one is `t`); a chunk inside the range is one uint4 store built from two aligned uint4 loads,
// a chunk at an edge stores its bytes one by one.  src_end: end of the readable source buffer.
// Every buffer a segment is copied between is device global memory, and the copy says so: its pointers carry the global
// address space, and a chunk is addressed by its OFFSET from dst / src.  (Addresses rebuilt from integers, as this code
// had them, or plain pointer parameters of an out-of-line function are generic: each access was a flat one.)
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef uint32_t g_u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) g_u32x4_t g_u32x4;
__device__ __forceinline__ uint4 funnel16(const g_u8* s, uint32_t q) {
    const g_u8* blk = s - q;
    const g_u32x4_t lo = *reinterpret_cast<const g_u32x4*>(blk);
    if (q == 0) return make_uint4(lo.x, lo.y, lo.z, lo.w);
    const g_u32x4_t hi = *reinterpret_cast<const g_u32x4*>(blk + 16);
    const uint32_t sh = q & 3u;
    uint32_t w0, w1, w2, w3, w4;
    switch (q >> 2) {  // (one value for the whole segment: a uniform branch)
        case 0: w0 = lo.x; w1 = lo.y; w2 = lo.z; w3 = lo.w; w4 = hi.x; break;
        case 1: w0 = lo.y; w1 = lo.z; w2 = lo.w; w3 = hi.x; w4 = hi.y; break;
        case 2: w0 = lo.z; w1 = lo.w; w2 = hi.x; w3 = hi.y; w4 = hi.z; break;
        default: w0 = lo.w; w1 = hi.x; w2 = hi.y; w3 = hi.z; w4 = hi.w; break;
    }
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                      __builtin_amdgcn_alignbyte(w4, w3, sh));
}

__device__ void copy_segment(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t len, const uint8_t* src_end, int64_t t,
                             int64_t nthr) {
    if (len <= 0) return;
    g_u8* const gd = (g_u8*)dst;
    const g_u8* const gs = (const g_u8*)src;
    const g_u8* const gend = (const g_u8*)src_end;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)len;
    const uintptr_t c0 = d0 & ~(uintptr_t)15, c1 = (d1 + 15) & ~(uintptr_t)15;
    const int64_t nchunk = (int64_t)((c1 - c0) >> 4);
    const int64_t e0 = -(int64_t)(d0 & 15);  // the first chunk starts this far from dst (0 .. -15)
    const uint32_t q = (uint32_t)(((uintptr_t)src - (uintptr_t)dst) & 15u);
    constexpr int U = 4;  // chunks in flight per thread
    for (int64_t i0 = t; i0 < nchunk; i0 += U * nthr) {
        uint4 v[U];
        bool full[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + (int64_t)u * nthr;
            const int64_t o = e0 + (i << 4);  // the chunk's offset from dst, and of its source bytes from src
            const g_u8* s = gs + o;
            full[u] = i < nchunk && o >= 0 && o + 16 <= len && (s - q) + (q ? 32 : 16) <= gend;
            if (full[u]) v[u] = funnel16(s, q);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + (int64_t)u * nthr;
            if (i >= nchunk) break;
            const int64_t o = e0 + (i << 4);
            if (full[u]) {
                g_u32x4_t w;
                w.x = v[u].x; w.y = v[u].y; w.z = v[u].z; w.w = v[u].w;
                *reinterpret_cast<g_u32x4*>(gd + o) = w;
            } else {  // an edge of the segment (or a source chunk at the end of its buffer)
                for (int b = 0; b < 16; ++b) {
                    const int64_t d = o + b;
                    if (d >= 0 && d < len) gd[d] = gs[d];
                }
            }
        }
    }
}

// One wave: frame `fr` of L bytes with its number rewritten to v, at fd (lane 0 builds the new header in registers and the
// CRC-16 from the identity crc_new = crc_old ^ (crc(H_old) ^ crc(H_new)) x^(8 |P|) mod G; the wave moves the payload).
// src_end: end of the buffer that holds fr.
__device__ __forceinline__ void renumber_frame_wave(uint8_t* fd, const uint8_t* fr, int64_t L, uint64_t v, const uint8_t* src_end, int lane) {
    uint32_t hw0 = 0, hw1 = 0, hw2 = 0, hw3 = 0, crc_new = 0;
    int h_old = 0, h_new = 0;
    if (lane == 0) {
        const uint8_t lead = fr[4];
        int u = 0;
        while (u < 7 && (lead & (0x80u >> u))) ++u;
        u = u ? u : 1;
        const int code = fr[2] >> 4;
        const int extra = (code == 6) ? 1 : (code == 7) ? 2 : 0;
        h_old = 4 + u + extra + 1;
        const int un = utf8_bytes(v);
        // the new header, byte i in bits 8 (i & 3) of hw(i >> 2): registers, not a private array in scratch
        auto setb = [&](int i, uint32_t b8) {
            const uint32_t sh = 8u * (uint32_t)(i & 3), m = ~(0xFFu << sh), b = (b8 & 0xFFu) << sh;
            if (i < 4) hw0 = (hw0 & m) | b; else if (i < 8) hw1 = (hw1 & m) | b; else if (i < 12) hw2 = (hw2 & m) | b; else hw3 = (hw3 & m) | b;
        };
        auto getb = [&](int i) -> uint8_t {
            const uint32_t w = (i < 4) ? hw0 : (i < 8) ? hw1 : (i < 12) ? hw2 : hw3;
            return (uint8_t)(w >> (8 * (i & 3)));
        };
        for (int i = 0; i < 4; ++i) setb(i, fr[i]);
        if (un == 1) {
            setb(4, (uint32_t)v);
        } else {
            setb(4, ((0xFF00u >> un) & 0xFFu) | (uint32_t)(v >> (6 * (un - 1))));
            for (int i = 1; i < un; ++i) setb(4 + i, 0x80u | (uint32_t)((v >> (6 * (un - 1 - i))) & 0x3Fu));
        }
        for (int i = 0; i < extra; ++i) setb(4 + un + i, fr[4 + u + i]);
        h_new = 4 + un + extra + 1;
        uint8_t c8 = 0;
        uint16_t ch_old = 0, ch_new = 0;
        for (int i = 0; i < h_new - 1; ++i) c8 = crc8_byte(c8, getb(i));
        setb(h_new - 1, c8);
        for (int i = 0; i < h_old; ++i) ch_old = crc16_byte(ch_old, fr[i]);
        for (int i = 0; i < h_new; ++i) ch_new = crc16_byte(ch_new, getb(i));
        const uint32_t crc_old = ((uint32_t)fr[L - 2] << 8) | fr[L - 1];
        crc_new = crc_old ^ crc16_mulmod((uint32_t)(ch_old ^ ch_new), crc16_xpow8((uint64_t)(L - 2 - h_old)));
    }
    h_old = __shfl(h_old, 0, 64);
    h_new = __shfl(h_new, 0, 64);
    hw0 = (uint32_t)__shfl((int)hw0, 0, 64);
    hw1 = (uint32_t)__shfl((int)hw1, 0, 64);
    hw2 = (uint32_t)__shfl((int)hw2, 0, 64);
    hw3 = (uint32_t)__shfl((int)hw3, 0, 64);
    if (lane < h_new) {
        const uint32_t w = (lane < 4) ? hw0 : (lane < 8) ? hw1 : (lane < 12) ? hw2 : hw3;
        fd[lane] = (uint8_t)(w >> (8 * (lane & 3)));
    }
    copy_segment(fd + h_new, fr + h_old, L - 2 - h_old, src_end, lane, 64);
    if (lane == 0) {
        fd[h_new + L - 2 - h_old] = (uint8_t)(crc_new >> 8);
        fd[h_new + L - 1 - h_old] = (uint8_t)crc_new;
    }
}

__device__ __forceinline__ void store_be64(uint8_t* p, uint64_t v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (56 - 8 * i));
}

// grid: n_stream * parts workgroups of 256; workgroup (s, p) copies its share of stream s's verbatim bytes and rewrites its
// share of the suffix seek points, its waves renumber the new frames k = 4p + wave, 4p + wave + 4 parts, ..., and (p == 0)
// writes the fixed header and the new seek points.  Every offset read from the old stream here was bounded by the size
// kernel (off0 <= off1 <= body); the suffix points' offsets are rewritten, never read through.  Where there is a suffix
// the frame count is unchanged (the plan's precondition), so a suffix point or frame keeps its number and its index.
__global__ __launch_bounds__(256) void splice_kernel(SpliceArgs a) {
    const int64_t s = (int64_t)blockIdx.x / a.parts;
    const int p = (int)((int64_t)blockIdx.x - s * a.parts);
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)p * 256 + tid, nthr = (int64_t)a.parts * 256;
    uint8_t* const dst = a.out + a.starts[s];
    const uint8_t* const osrc = a.old + a.old_starts[s];
    const uint8_t* const old_end = a.old + a.old_bytes;
    const int64_t on = a.old_nbytes[s];
    const int64_t j = splice_row(a, s);
    if (j < 0) {
        copy_segment(dst, osrc, on, old_end, t, nthr);
        return;
    }
    const int64_t nfe = splice_nfe(a);
    const int64_t hb = stream_header_bytes(a.nf_new), hb_old = stream_header_bytes(a.nf_old), hb_enc = stream_header_bytes(nfe);
    const uint8_t* const esrc = a.enc + a.enc_starts[j];
    const int64_t enc_body = a.enc_nbytes[j] - hb_enc;
    const int64_t o0 = a.off0[s], o1 = a.off1[s];
    const int64_t new_mid = enc_body + append_growth(a.f0, nfe);
    const int64_t delta = new_mid - (o1 - o0);
    // verbatim: the seek points and frames in front of the span, the frames behind it
    copy_segment(dst + 46, osrc + 46, 18 * a.f0, old_end, t, nthr);
    copy_segment(dst + hb, osrc + hb_old, o0, old_end, t, nthr);
    copy_segment(dst + hb + o0 + new_mid, osrc + hb_old + o1, (on - hb_old) - o1, old_end, t, nthr);
    // the seek points behind the span: sample number and count copied, offset moved by delta
    for (int64_t k = a.f1 + t; k < a.nf_old; k += nthr) {
        const uint8_t* sp = osrc + 46 + 18 * k;
        uint8_t* pt = dst + 46 + 18 * k;
#pragma unroll
        for (int i = 0; i < 8; ++i) pt[i] = sp[i];
        store_be64(pt + 8, (uint64_t)((int64_t)load_be64(sp + 8) + delta));
        pt[16] = sp[16];
        pt[17] = sp[17];
    }
    if (p == 0) {
        for (int i = tid; i < 46; i += 256) dst[i] = stream_header_byte(i, a.B, a.nch, a.size_new, a.nf_new);  // (no MD5: the samples changed)
        for (int64_t k = tid; k < nfe; k += 256) {  // the new seek points: sample, offset, samples (big-endian)
            uint8_t* pt = dst + 46 + 18 * (a.f0 + k);
            store_be64(pt, (uint64_t)(a.f0 + k) * (uint64_t)a.B);
            store_be64(pt + 8, (uint64_t)(o0 + (int64_t)load_be64(esrc + 46 + 18 * k + 8) + append_growth(a.f0, k)));
            pt[16] = esrc[46 + 18 * k + 16];
            pt[17] = esrc[46 + 18 * k + 17];
        }
    }
    // the new frames, one per wave at a time
    const int wave = tid >> 6, lane = tid & 63;
    for (int64_t k = (int64_t)p * 4 + wave; k < nfe; k += (int64_t)a.parts * 4) {
        const int64_t off = (int64_t)load_be64(esrc + 46 + 18 * k + 8);
        const int64_t end = (k + 1 < nfe) ? (int64_t)load_be64(esrc + 46 + 18 * (k + 1) + 8) : enc_body;
        renumber_frame_wave(dst + hb + o0 + off + append_growth(a.f0, k), esrc + hb_enc + off, end - off, (uint64_t)(a.f0 + k), a.enc + a.enc_bytes, lane);
    }
}

}  // namespace fa
