// append_kernels.hpp -- FlacArray.append on gfx950: extend every stream of a store by new samples without re-encoding it.
//
// The frames of concat(a, b) are the frames of a followed by the frames of (tail of a) + b (every frame is analysed from
// its own samples).  So the appended store is spliced from two stores: the old one (a) and a fresh encode of the old
// short tail and the new samples, whose frames are renumbered.  Per stream the result is
//     [ fLaC + STREAMINFO + SEEKTABLE of base + F' points ][ kept old frames, verbatim ][ F' new frames, renumbered ]
// base = the old stream's full frames; F' = the new encode's frames.  Renumbering changes a frame's UTF-8 number field
// (its length may grow), its header CRC-8 and its CRC-16; the CRC-16 is linear (poly 0x8005, zero init, no final xor):
//     crc(H || P) = crc(H) * x^(8|P|) + crc(P)  mod G,  so  crc_new = crc_old ^ (crc(H_old) ^ crc(H_new)) * x^(8|P|) mod G
// -- O(log |P|) work per frame, no pass over its payload.  All streams share their frame numbers, so the growth of the
// number fields is one constant for every stream (append_growth), and each stream's new size is a sum of sizes the
// device already holds (append_size_kernel).  The copy is one launch (append_splice_kernel): 16-byte destination
// chunks, each assembled from two aligned 16-byte source loads by a byte funnel shift (the source/destination
// misalignment of a segment is one value for all its chunks), plain vector stores; only the edges of a segment and the
// few computed header bytes are stored byte by byte.
//
// K10a quantise_rows_kernel: float32 / float64 samples quantised with GIVEN per-stream offsets and gains (utils.c:229-240,
//      :316-323: the arithmetic of quantise_f32 / quantise_f64), written at a row stride of the caller's choice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_kernels.hpp"  // (load_be64)
#include "encode_placed.hpp"
#include "quantize_kernels.hpp"

namespace fa {

// ---- K10a ----------------------------------------------------------------------------------------
template <typename F, typename I>
__device__ __forceinline__ I quantise_given(F x, F off, F gain);
template <>
__device__ __forceinline__ int32_t quantise_given<float, int32_t>(float x, float off, float gain) { return quantise_f32(x, off, gain); }
template <>
__device__ __forceinline__ int64_t quantise_given<double, int64_t>(double x, double off, double gain) { return quantise_f64(x, off, gain); }

// grid-stride over n_stream * n samples; out[s * out_stride + i] (a row stride > n writes into a wider image)
template <typename F, typename I>
__global__ __launch_bounds__(256) void quantise_rows_kernel(const F* __restrict__ in, int64_t n_stream, int64_t n, const F* __restrict__ offsets,
                                                            const F* __restrict__ gains, I* __restrict__ out, int64_t out_stride,
                                                            int* __restrict__ flags) {
    const int64_t total = n_stream * n;
    bool nan = false;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t s = g / n;
        const int64_t i = g - s * n;
        const F x = in[g];
        nan = nan || (x != x);
        out[s * out_stride + i] = quantise_given<F, I>(x, offsets[s], gains[s]);
    }
    if (nan) atomicOr(flags, 1);
}

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

struct AppendArgs {
    const uint8_t* old;  // the old store
    int64_t old_bytes;
    const int64_t* old_starts;
    const int64_t* old_nbytes;
    const uint8_t* enc;  // the encode of tail + new samples
    int64_t enc_bytes;
    const int64_t* enc_starts;
    const int64_t* enc_nbytes;
    int64_t* kept;       // per stream: bytes of the kept old frames (written by the size kernel)
    const int64_t* starts;  // the new store
    int64_t* nbytes;
    uint8_t* out;
    int64_t capacity;
    int* err;
    int64_t n_stream, old_size, new_size, base, nf_old, nf_enc;
    int32_t B, nch, parts;
};

// ---- K10b: per stream, the new size (and the kept old bytes); checks the layout both stores must have -------------
// The old stream must be one this encoder wrote for THIS call: "fLaC", STREAMINFO first and not last with block size B,
// the call's channel count and the call's stream size (the 36-bit total), the SEEKTABLE last with one point per frame.
// Returns false otherwise; *kept = the bytes of its kept frames (all frames but a short last one).
__device__ __forceinline__ bool old_stream_kept(const AppendArgs& a, int64_t s, int64_t* kept) {
    const int64_t hb_old = stream_header_bytes(a.nf_old);
    const int64_t os = a.old_starts[s], on = a.old_nbytes[s];
    *kept = 0;
    if (os < 0 || on < hb_old || os + on > a.old_bytes) return false;
    const uint8_t* h = a.old + os;
    const uint32_t stl = ((uint32_t)h[43] << 16) | ((uint32_t)h[44] << 8) | h[45];
    const uint64_t packed = load_be64(h + 18);  // rate 20 | channels - 1: 3 | bits - 1: 5 | total samples: 36
    const uint64_t total = ((uint64_t)a.old_size < (1ULL << 36)) ? (uint64_t)a.old_size : 0;
    if (h[0] != 'f' || h[1] != 'L' || h[2] != 'a' || h[3] != 'C' || h[4] != 0 || h[42] != 0x83 || stl != 18u * (uint32_t)a.nf_old ||
        h[8] != (uint8_t)(a.B >> 8) || h[9] != (uint8_t)a.B || (int)((packed >> 41) & 7u) + 1 != a.nch ||
        (packed & ((1ULL << 36) - 1)) != total)
        return false;
    const int64_t k = (a.base < a.nf_old) ? (int64_t)load_be64(h + 46 + 18 * a.base + 8) : on - hb_old;
    if (k < 0 || k > on - hb_old) return false;
    *kept = k;
    return true;
}

// before anything is decoded or encoded: is every old stream one the call can extend?
__global__ __launch_bounds__(256) void append_check_kernel(AppendArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t kept;
    if (s < a.n_stream && !old_stream_kept(a, s, &kept)) atomicOr(a.err, 2);
}

__global__ __launch_bounds__(256) void append_size_kernel(AppendArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_stream) return;
    const int64_t hb_enc = stream_header_bytes(a.nf_enc);
    const int64_t es = a.enc_starts[s], en = a.enc_nbytes[s];
    int64_t kept;
    if (!old_stream_kept(a, s, &kept) || es < 0 || en < hb_enc || es + en > a.enc_bytes) {
        atomicOr(a.err, 2);
        kept = 0;
    }
    a.kept[s] = kept;
    a.nbytes[s] = stream_header_bytes(a.base + a.nf_enc) + kept + (en - hb_enc) + append_growth(a.base, a.nf_enc);
}

// ---- K10c: the copy --------------------------------------------------------------------------------------------
// Copy [src, src + len) to [dst, dst + len): the 16-byte destination chunks that meet the range are shared out over
// `nthr` threads (this one is `t`); a chunk inside the range is one uint4 store built from two aligned uint4 loads,
// a chunk at an edge stores its bytes one by one.  src_end: end of the readable source buffer.
__device__ __forceinline__ uint4 funnel16(const uint8_t* s, uint32_t q) {
    const uint8_t* blk = s - q;
    const uint4 lo = *reinterpret_cast<const uint4*>(blk);
    if (q == 0) return lo;
    const uint4 hi = *reinterpret_cast<const uint4*>(blk + 16);
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
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)len;
    const uintptr_t c0 = d0 & ~(uintptr_t)15, c1 = (d1 + 15) & ~(uintptr_t)15;
    const int64_t nchunk = (int64_t)((c1 - c0) >> 4);
    const int64_t delta = reinterpret_cast<intptr_t>(src) - reinterpret_cast<intptr_t>(dst);
    const uint32_t q = (uint32_t)(((uintptr_t)src - (uintptr_t)dst) & 15u);
    constexpr int U = 4;  // chunks in flight per thread
    for (int64_t i0 = t; i0 < nchunk; i0 += U * nthr) {
        uint4 v[U];
        bool full[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + (int64_t)u * nthr;
            const uintptr_t c = c0 + ((uintptr_t)i << 4);
            const uint8_t* s = reinterpret_cast<const uint8_t*>((intptr_t)c + delta);
            full[u] = i < nchunk && c >= d0 && c + 16 <= d1 && (s - q) + (q ? 32 : 16) <= src_end;
            if (full[u]) v[u] = funnel16(s, q);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + (int64_t)u * nthr;
            if (i >= nchunk) break;
            const uintptr_t c = c0 + ((uintptr_t)i << 4);
            if (full[u]) {
                *reinterpret_cast<uint4*>(c) = v[u];
            } else {  // an edge of the segment (or a source chunk at the end of its buffer)
                for (int b = 0; b < 16; ++b) {
                    const uintptr_t d = c + (uintptr_t)b;
                    if (d >= d0 && d < d1) *reinterpret_cast<uint8_t*>(d) = *reinterpret_cast<const uint8_t*>((intptr_t)d + delta);
                }
            }
        }
    }
}

// grid: n_stream * parts workgroups of 256; workgroup (s, p) copies its share of stream s's kept old bytes and seek
// points, its waves renumber the new frames k = 4p + wave, 4p + wave + 4 parts, ..., and (p == 0) writes the fixed header
// and the new seek points.
__global__ __launch_bounds__(256) void append_splice_kernel(AppendArgs a) {
    const int64_t s = (int64_t)blockIdx.x / a.parts;
    const int p = (int)((int64_t)blockIdx.x - s * a.parts);
    const int tid = threadIdx.x;
    const int64_t nf = a.base + a.nf_enc;
    const int64_t hb = stream_header_bytes(nf), hb_old = stream_header_bytes(a.nf_old), hb_enc = stream_header_bytes(a.nf_enc);
    uint8_t* const dst = a.out + a.starts[s];
    const uint8_t* const osrc = a.old + a.old_starts[s];
    const uint8_t* const esrc = a.enc + a.enc_starts[s];
    const int64_t kept = a.kept[s];
    const int64_t enc_body = a.enc_nbytes[s] - hb_enc;
    const int64_t t = (int64_t)p * 256 + tid, nthr = (int64_t)a.parts * 256;
    // the kept seek points and frames of the old stream: verbatim
    copy_segment(dst + 46, osrc + 46, 18 * a.base, a.old + a.old_bytes, t, nthr);
    copy_segment(dst + hb, osrc + hb_old, kept, a.old + a.old_bytes, t, nthr);
    if (p == 0) {
        for (int i = tid; i < 46; i += 256) dst[i] = stream_header_byte(i, a.B, a.nch, a.new_size, nf);
        for (int64_t k = tid; k < a.nf_enc; k += 256) {  // the new seek points: sample, offset, samples (big-endian)
            const uint64_t sn = (uint64_t)(a.base + k) * (uint64_t)a.B;
            const uint64_t off = (uint64_t)(kept + (int64_t)load_be64(esrc + 46 + 18 * k + 8) + append_growth(a.base, k));
            const uint32_t ns = ((uint32_t)esrc[46 + 18 * k + 16] << 8) | esrc[46 + 18 * k + 17];
            uint8_t* pt = dst + 46 + 18 * (a.base + k);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pt[i] = (uint8_t)(sn >> (56 - 8 * i));
                pt[8 + i] = (uint8_t)(off >> (56 - 8 * i));
            }
            pt[16] = (uint8_t)(ns >> 8);
            pt[17] = (uint8_t)ns;
        }
    }
    // the new frames, one per wave at a time: lane 0 rewrites the header and the CRC-16, the wave moves the payload
    const int wave = tid >> 6, lane = tid & 63;
    for (int64_t k = (int64_t)p * 4 + wave; k < a.nf_enc; k += (int64_t)a.parts * 4) {
        const int64_t off = (int64_t)load_be64(esrc + 46 + 18 * k + 8);
        const int64_t end = (k + 1 < a.nf_enc) ? (int64_t)load_be64(esrc + 46 + 18 * (k + 1) + 8) : enc_body;
        const uint8_t* fr = esrc + hb_enc + off;
        const int64_t L = end - off;
        uint8_t* fd = dst + hb + kept + off + append_growth(a.base, k);
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
            const uint64_t v = (uint64_t)(a.base + k);
            const int un = utf8_bytes(v);
            // the new header, byte i in bits 8 (i & 3) of hw(i >> 2): registers, not a private array in scratch
            auto setb = [&](int i, uint32_t v) {
                const uint32_t sh = 8u * (uint32_t)(i & 3), m = ~(0xFFu << sh), b = (v & 0xFFu) << sh;
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
        copy_segment(fd + h_new, fr + h_old, L - 2 - h_old, a.enc + a.enc_bytes, lane, 64);
        if (lane == 0) {
            fd[h_new + L - 2 - h_old] = (uint8_t)(crc_new >> 8);
            fd[h_new + L - 1 - h_old] = (uint8_t)crc_new;
        }
    }
}

}  // namespace fa
