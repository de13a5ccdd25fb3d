// window_kernels.hpp -- K14, FlacArray.window and FlacArray.trim on gfx950: cut samples [first, last) of some or all
// streams out of a store as a store of its own, without re-encoding the frames that are kept whole.
//
// A frame is analysed from its own samples only (splice_kernels.hpp), so for first = f0 B the frames of x[:, first:last]
// ARE the frames f0, f0 + 1, ... of x with their numbers lowered by f0.  With nk the old frames kept (all of them up to
// the old end when last is the old stream size, else (last - first) / B) and, where last falls inside an old frame, one
// freshly encoded short frame of the r = (last - first) % B samples in front of the cut (the host decodes and encodes it
// as the splice obtains its span encode), the result has nf_new = nk + tail frames and is, per picked stream,
//     [ 46 header bytes of last - first samples and nf_new frames, MD5 zero ]
//     [ nk seek points: sample k B, offset off_old(f0 + k) - off_old(f0) - append_growth(f0, k), count copied ][ tail point ]
//     [ nk old frames renumbered f0 + k -> k ][ the tail frame renumbered 0 -> nk ]
// append_growth(f0, k) is exactly the number of header bytes the frames [f0, f0 + k) lose when renumbered to [0, k):
// all streams share their frame numbers, so every destination offset is a closed form of the old seek table -- no scan.
// Renumbering is renumber_frame_wave of the splice (number field, CRC-8, CRC-16 by the linear identity); the payloads
// move through copy_segment.  Two shortcuts: f0 == 0 (truncate only) renumbers nothing, the kept points and frames are
// two copy_segments; a window that is the whole stream is one copy_segment of the stream, STREAMINFO MD5 included
// (pure stream selection).
//
// K14a window_check_kernel  one thread per (picked stream, checked frame): the stream index in range and not named
//                           twice, the layout test of old_stream_kept, and EVERY seek offset of the frames f0 ..
//                           f0 + nchk - 1 (the kept ones and the one the tail is decoded from): ordered, inside the body,
//                           each frame at least 13 bytes and at least its own header plus the CRC-16, its number field as
//                           long as its number's; gathers the picked streams' (start, nbytes) for the tail decode.  Runs
//                           before anything is decoded or copied; nothing later reads outside [frame start, frame end)
//                           of a checked frame.
// K14b window_size_kernel   one thread per picked stream: the new size (starts_scan_kernel follows, as for the splice).
// K14c window_kernel        one launch, `parts` workgroups of 256 per picked stream (~64 KB of output each), no
//                           dependencies between workgroups, plain vector and byte stores.
#pragma once
#include "splice_kernels.hpp"

namespace fa {

constexpr int kWindowBadLayout = 2;  // a picked stream is not one this encoder wrote for the call's geometry
constexpr int kWindowBadIndex = 4;   // a stream index out of range or named twice
constexpr int kWindowBadTable = 8;   // a seek offset out of order or outside the body, a frame shorter than header + CRC-16
constexpr int64_t kWindowMinFrame = 13;  // the smallest frame this encoder writes: a constant one-channel subframe

struct WindowArgs {
    const uint8_t* old;  // the old store
    int64_t old_bytes;
    const int64_t* old_starts;
    const int64_t* old_nbytes;
    const int64_t* sidx;  // [m] flat indices of the picked streams, in output order; NULL: all streams
    int32_t* slot;        // [n_stream], all -1 before the check: the output row of a stream (unused when sidx is NULL)
    int64_t* sub_starts;  // [m] the picked streams' starts and sizes (the tail decode's index)
    int64_t* sub_nbytes;
    const uint8_t* enc;  // the one-frame encode of the tail image, m streams (NULL without a tail)
    int64_t enc_bytes;
    const int64_t* enc_starts;
    const int64_t* enc_nbytes;
    const int64_t* starts;  // the new store, m streams
    int64_t* nbytes;
    uint8_t* out;
    int* err;  // kWindowBad*
    int64_t n_stream, m, size_old, size_new, f0, nk, nchk, nf_old, nf_new;
    int32_t B, nch, parts, tail, whole;
};

// what old_stream_kept reads of a splice's arguments
__device__ __forceinline__ SpliceArgs window_as_splice(const WindowArgs& a) {
    SpliceArgs s;
    s.old = a.old; s.old_bytes = a.old_bytes; s.old_starts = a.old_starts; s.old_nbytes = a.old_nbytes;
    s.size_old = a.size_old; s.nf_old = a.nf_old; s.B = a.B; s.nch = a.nch;
    return s;
}

__device__ __forceinline__ int64_t window_stream(const WindowArgs& a, int64_t j) { return a.sidx ? a.sidx[j] : j; }

// offset of old frame f from the first frame (the body's end stands in for frame nf_old); h: the stream's first byte
__device__ __forceinline__ int64_t window_off(const WindowArgs& a, const uint8_t* h, int64_t on, int64_t f) {
    return (f < a.nf_old) ? (int64_t)load_be64(h + 46 + 18 * f + 8) : on - stream_header_bytes(a.nf_old);
}

// bytes of a frame header whose first five bytes are fr[0..4], CRC-8 included (as renumber_frame_wave counts them);
// *u: the bytes of its number field
__device__ __forceinline__ int window_header_len(const uint8_t* fr, int* u) {
    const uint8_t lead = fr[4];
    int n = 0;
    while (n < 7 && (lead & (0x80u >> n))) ++n;
    n = n ? n : 1;
    *u = n;
    const int code = fr[2] >> 4;
    return 4 + n + ((code == 6) ? 1 : (code == 7) ? 2 : 0) + 1;
}

// ---- K14a (slot is all -1 before the launch; sub_starts / sub_nbytes are zero) ------------------------------------------
__global__ __launch_bounds__(256) void window_check_kernel(WindowArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.m * a.nchk) return;
    const int64_t j = t / a.nchk, k = t - j * a.nchk;
    int64_t s = j;
    if (a.sidx) {
        s = a.sidx[j];
        if (s < 0 || s >= a.n_stream) {
            if (k == 0) atomicOr(a.err, kWindowBadIndex);
            return;
        }
        if (k == 0 && atomicExch(&a.slot[s], (int32_t)j) != -1) {
            atomicOr(a.err, kWindowBadIndex);
            return;
        }
    }
    // the layout, before a seek point is read: every thread of the stream tests it, thread 0 reports it
    const SpliceArgs sa = window_as_splice(a);
    int64_t unused;
    if (!old_stream_kept(sa, s, a.nf_old, &unused)) {
        if (k == 0) atomicOr(a.err, kWindowBadLayout);
        return;
    }
    if (k == 0) {
        a.sub_starts[j] = a.old_starts[s];
        a.sub_nbytes[j] = a.old_nbytes[s];
    }
    if (a.whole) return;  // copied as it is: no offset of its table is followed
    const uint8_t* h = a.old + a.old_starts[s];
    const int64_t on = a.old_nbytes[s], body = on - stream_header_bytes(a.nf_old);
    const int64_t f = a.f0 + k;  // (< nf_old: the host's plan)
    const int64_t off = window_off(a, h, on, f), end = window_off(a, h, on, f + 1);
    bool ok = off >= 0 && end <= body && off <= end && end - off >= kWindowMinFrame && (f != 0 || off == 0);
    if (ok) {
        // the frame holds its header and CRC-16, and its number field has the length of number f: the destination
        // offsets (append_growth) count on it
        int u;
        const int hl = window_header_len(h + stream_header_bytes(a.nf_old) + off, &u);
        ok = end - off >= (int64_t)hl + 2 && u == utf8_bytes((uint64_t)f);
    }
    if (!ok) atomicOr(a.err, kWindowBadTable);
}

// ---- K14b ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_size_kernel(WindowArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const int64_t s = window_stream(a, j);
    const int64_t on = a.old_nbytes[s];
    int64_t size = on;
    if (!a.whole) {
        const uint8_t* h = a.old + a.old_starts[s];
        size = stream_header_bytes(a.nf_new) + window_off(a, h, on, a.f0 + a.nk) - window_off(a, h, on, a.f0) - append_growth(a.f0, a.nk);
        if (a.tail) {
            const int64_t es = a.enc_starts[j], en = a.enc_nbytes[j], hb_enc = stream_header_bytes(1);
            if (es < 0 || en < hb_enc + kWindowMinFrame || es + en > a.enc_bytes) {
                atomicOr(a.err, kWindowBadLayout);
                size = 0;
            } else {
                size += (en - hb_enc) + (utf8_bytes((uint64_t)a.nk) - 1);
            }
        }
    }
    a.nbytes[j] = size;
}

// ---- K14c ---------------------------------------------------------------------------------------------------------------
// grid: m * parts workgroups of 256.  Workgroup (j, p) writes its share of output stream j: (p == 0) the fixed header;
// all parts share out the seek points; their waves take the kept frames k = 4p + wave, + 4 parts, ... through
// renumber_frame_wave with number k; the last part's wave 0 renumbers the tail frame 0 -> nk from the encode's buffer.
// Every offset followed here was bounded by the check kernel for exactly the frames f0 .. f0 + nk.
__global__ __launch_bounds__(256) void window_kernel(WindowArgs a) {
    const int64_t j = (int64_t)blockIdx.x / a.parts;
    const int p = (int)((int64_t)blockIdx.x - j * a.parts);
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)p * 256 + tid, nthr = (int64_t)a.parts * 256;
    const int64_t s = window_stream(a, j);
    uint8_t* const dst = a.out + a.starts[j];
    const uint8_t* const osrc = a.old + a.old_starts[s];
    const uint8_t* const old_end = a.old + a.old_bytes;
    const int64_t on = a.old_nbytes[s];
    if (a.whole) {  // pure stream selection: the stream as it is, its signature included
        copy_segment(dst, osrc, on, old_end, t, nthr);
        return;
    }
    const int64_t hb = stream_header_bytes(a.nf_new), hb_old = stream_header_bytes(a.nf_old);
    const int64_t o0 = window_off(a, osrc, on, a.f0), o1 = window_off(a, osrc, on, a.f0 + a.nk);
    const int64_t kept = o1 - o0 - append_growth(a.f0, a.nk);  // bytes of the kept frames in the new stream
    const int wave = tid >> 6, lane = tid & 63;
    if (p == 0)
        for (int i = tid; i < 46; i += 256) dst[i] = stream_header_byte(i, a.B, a.nch, a.size_new, a.nf_new);  // (no MD5: other samples)
    if (a.f0 == 0) {
        // truncate only: the points and frames in front of the cut keep their numbers and offsets (o0 == 0: checked)
        copy_segment(dst + 46, osrc + 46, 18 * a.nk, old_end, t, nthr);
        copy_segment(dst + hb, osrc + hb_old, o1, old_end, t, nthr);
    } else {
        for (int64_t k = t; k < a.nk; k += nthr) {  // the kept seek points: sample, offset, samples (big-endian)
            const uint8_t* sp = osrc + 46 + 18 * (a.f0 + k);
            uint8_t* pt = dst + 46 + 18 * k;
            store_be64(pt, (uint64_t)k * (uint64_t)a.B);
            store_be64(pt + 8, (uint64_t)((int64_t)load_be64(sp + 8) - o0 - append_growth(a.f0, k)));
            pt[16] = sp[16];
            pt[17] = sp[17];
        }
        // the kept frames, one per wave at a time
        for (int64_t k = (int64_t)p * 4 + wave; k < a.nk; k += (int64_t)a.parts * 4) {
            const int64_t off = window_off(a, osrc, on, a.f0 + k), end = window_off(a, osrc, on, a.f0 + k + 1);
            renumber_frame_wave(dst + hb + off - o0 - append_growth(a.f0, k), osrc + hb_old + off, end - off, (uint64_t)k, old_end, lane);
        }
    }
    if (a.tail && p == a.parts - 1 && wave == 0) {
        const uint8_t* const esrc = a.enc + a.enc_starts[j];
        const int64_t hb_enc = stream_header_bytes(1);
        if (lane == 0) {
            uint8_t* pt = dst + 46 + 18 * a.nk;
            store_be64(pt, (uint64_t)a.nk * (uint64_t)a.B);
            store_be64(pt + 8, (uint64_t)kept);
            pt[16] = esrc[46 + 16];
            pt[17] = esrc[46 + 17];
        }
        renumber_frame_wave(dst + hb + kept, esrc + hb_enc, a.enc_nbytes[j] - hb_enc, (uint64_t)a.nk, a.enc + a.enc_bytes, lane);
    }
}

}  // namespace fa
