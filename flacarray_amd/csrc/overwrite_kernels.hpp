// overwrite_kernels.hpp -- K11, FlacArray.overwrite on gfx950: replace samples [first, first + n) of some or all streams of
// a store without re-encoding the rest of it.
//
// A frame is analysed from its own samples only, so new samples in [first, first + n) change the frames f0 .. f1 - 1 that
// overlap the range (f0 = first / B, f1 = min(F, ceil((first + n) / B))) and no other.  The span [f0 B, min(f1 B, N))
// starts on a frame boundary and ends on one or at the end of the stream, so a one-shot encode of the patched span image
// IS those frames, numbered from 0.  Per participating stream the result is
//     [ 46 header bytes, MD5 zero ][ seek points < f0 ][ new points ][ points >= f1, offset + delta ]
//     [ frames < f0, verbatim ][ f1 - f0 new frames, renumbered k -> f0 + k ][ frames >= f1, verbatim, moved by delta ]
// with delta = new_mid - old_mid the change in the bytes of the middle frames; a stream that does not take part is copied
// whole.  Frame count and the numbers of the suffix frames do not change, so the suffix is a byte copy at a per-stream
// misalignment (copy_segment / funnel16 of K10c); the new frames are renumbered as K10c renumbers (UTF-8 number, CRC-8,
// CRC-16 through the linear identity), and their header growth is K10's closed form append_growth(f0, k).
//
// K11a overwrite_check_kernel   one thread per participating stream: index in range and not named twice, the layout checks
//                               of old_stream_kept, the seek offsets of f0 and f1 ordered and inside the body; gathers the
//                               participating streams' (start, nbytes) for the span decode.  Runs before anything is decoded.
// K11b overwrite_size_kernel    one thread per stream: the new size, and off_old(f0) / off_old(f1) for the splice.
// K11c overwrite_splice_kernel  one launch, `parts` workgroups per stream (~64 KB of output each), no dependencies between
//                               workgroups, plain vector and byte stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "append_kernels.hpp"  // (copy_segment, funnel16, crc16_mulmod, crc16_xpow8, utf8_bytes, append_growth, old_stream_kept)

namespace fa {

struct OverwriteArgs {
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
    int64_t n_stream, m, size, f0, f1, nf;
    int32_t B, nch, parts;
};

// off_old(f0) and off_old(f1) of old stream s (the body's end stands in for frame nf), after the layout checks of K10b:
// both inside the body and ordered, or false.
__device__ __forceinline__ bool overwrite_bounds(const OverwriteArgs& a, int64_t s, int64_t* o0, int64_t* o1) {
    AppendArgs k;
    k.old = a.old; k.old_bytes = a.old_bytes; k.old_starts = a.old_starts; k.old_nbytes = a.old_nbytes;
    k.old_size = a.size; k.nf_old = a.nf; k.B = a.B; k.nch = a.nch;
    k.base = a.f0;
    const bool ok0 = old_stream_kept(k, s, o0);
    k.base = a.f1;
    const bool ok1 = old_stream_kept(k, s, o1);
    return ok0 && ok1 && *o0 <= *o1;
}

__device__ __forceinline__ int64_t overwrite_row(const OverwriteArgs& a, int64_t s) { return a.sidx ? (int64_t)a.slot[s] : s; }

// ---- K11a (slot is all -1 before the launch) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void overwrite_check_kernel(OverwriteArgs a) {
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
    if (!overwrite_bounds(a, s, &o0, &o1)) {
        atomicOr(a.err, 2);
        return;
    }
    a.sub_starts[j] = a.old_starts[s];
    a.sub_nbytes[j] = a.old_nbytes[s];
}

// ---- K11b -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void overwrite_size_kernel(OverwriteArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_stream) return;
    const int64_t os = a.old_starts[s], on = a.old_nbytes[s];
    const int64_t j = overwrite_row(a, s);
    int64_t o0 = 0, o1 = 0, size = on;
    if (j < 0) {  // copied whole: the copy reads [os, os + on)
        if (os < 0 || on < 0 || os + on > a.old_bytes) {
            atomicOr(a.err, 2);
            size = 0;
        }
    } else {
        const int64_t hb_enc = stream_header_bytes(a.f1 - a.f0);
        const int64_t es = a.enc_starts[j], en = a.enc_nbytes[j];
        if (!overwrite_bounds(a, s, &o0, &o1) || es < 0 || en < hb_enc || es + en > a.enc_bytes) {
            atomicOr(a.err, 2);
            o0 = o1 = 0;
            size = 0;
        } else {
            size = on - (o1 - o0) + (en - hb_enc) + append_growth(a.f0, a.f1 - a.f0);
        }
    }
    a.off0[s] = o0;
    a.off1[s] = o1;
    a.nbytes[s] = size;
}

// ---- K11c -------------------------------------------------------------------------------------------------------------
// One wave: frame `fr` of L bytes with its number rewritten to v, at fd (K10c's renumbering: lane 0 builds the new header
// in registers and the CRC-16 from the identity crc_new = crc_old ^ (crc(H_old) ^ crc(H_new)) x^(8 |P|) mod G; the wave
// moves the payload).  src_end: end of the buffer that holds fr.
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
// kernel (off0 <= off1 <= body); the suffix points' offsets are rewritten, never read through.
__global__ __launch_bounds__(256) void overwrite_splice_kernel(OverwriteArgs a) {
    const int64_t s = (int64_t)blockIdx.x / a.parts;
    const int p = (int)((int64_t)blockIdx.x - s * a.parts);
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)p * 256 + tid, nthr = (int64_t)a.parts * 256;
    uint8_t* const dst = a.out + a.starts[s];
    const uint8_t* const osrc = a.old + a.old_starts[s];
    const uint8_t* const old_end = a.old + a.old_bytes;
    const int64_t on = a.old_nbytes[s];
    const int64_t j = overwrite_row(a, s);
    if (j < 0) {
        copy_segment(dst, osrc, on, old_end, t, nthr);
        return;
    }
    const int64_t nfe = a.f1 - a.f0;
    const int64_t hb = stream_header_bytes(a.nf), hb_enc = stream_header_bytes(nfe);
    const uint8_t* const esrc = a.enc + a.enc_starts[j];
    const int64_t enc_body = a.enc_nbytes[j] - hb_enc;
    const int64_t o0 = a.off0[s], o1 = a.off1[s];
    const int64_t new_mid = enc_body + append_growth(a.f0, nfe);
    const int64_t delta = new_mid - (o1 - o0);
    // verbatim: the seek points and frames in front of the span, the frames behind it
    copy_segment(dst + 46, osrc + 46, 18 * a.f0, old_end, t, nthr);
    copy_segment(dst + hb, osrc + hb, o0, old_end, t, nthr);
    copy_segment(dst + hb + o0 + new_mid, osrc + hb + o1, (on - hb) - o1, old_end, t, nthr);
    // the seek points behind the span: sample number and count copied, offset moved by delta
    for (int64_t k = a.f1 + t; k < a.nf; k += nthr) {
        const uint8_t* sp = osrc + 46 + 18 * k;
        uint8_t* pt = dst + 46 + 18 * k;
#pragma unroll
        for (int i = 0; i < 8; ++i) pt[i] = sp[i];
        store_be64(pt + 8, (uint64_t)((int64_t)load_be64(sp + 8) + delta));
        pt[16] = sp[16];
        pt[17] = sp[17];
    }
    if (p == 0) {
        for (int i = tid; i < 46; i += 256) dst[i] = stream_header_byte(i, a.B, a.nch, a.size, a.nf);  // (no MD5: the samples changed)
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
