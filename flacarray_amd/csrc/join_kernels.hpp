// join_kernels.hpp -- K15, FlacArray.concatenate and FlacArray.extend on gfx950: lay the streams of several stores behind
// one another along the sample axis as ONE store, without decoding a sample or re-encoding a frame.  The inverse of K14.
//
// A frame is analysed from its own samples only (splice_kernels.hpp), so when every part but the last is a whole number of
// blocks long the frames of concatenate(x_0, x_1, ...) ARE the frames of the parts with their numbers raised.  With parts
// p = 0 .. P-1 of N_p samples, nf_p = ceil(N_p / B) frames, base_p = (N_0 + ... + N_{p-1}) / B, nf_new = sum nf_p,
// N_new = sum N_p, hb(F) = 46 + 18 F, body_p(s) = nbytes_p(s) - hb(nf_p), growth_p = append_growth(base_p, nf_p) (the
// header bytes the frames of part p gain when renumbered to [base_p, base_p + nf_p): one value for all streams) and
//     D_p(s) = sum_{q < p} (body_q(s) + growth_q)
// the new stream s is
//     [ 46 header bytes of N_new samples and nf_new frames, MD5 zero ]
//     [ seek point base_p + k: sample (base_p + k) B, offset D_p(s) + off_p(s, k) + append_growth(base_p, k), count copied ]
//     [ frame k of part p renumbered to base_p + k at hb(nf_new) + that offset ]
// of hb(nf_new) + sum_p (body_p(s) + growth_p) bytes.  Every destination is a closed form of the parts' seek tables and
// one short per-stream prefix sum over the parts (join_size_kernel); nothing is scanned over frames.  Renumbering is
// renumber_frame_wave of the splice (number field, CRC-8, CRC-16 by the linear identity), payloads move through
// copy_segment.  Two shortcuts: part 0 (base 0) changes neither numbers nor offsets, so its seek points and its whole body
// are two copy_segments -- a large store extended by a small one moves at copy speed; a single part is one copy_segment
// per stream, STREAMINFO MD5 included.
//
// The part descriptors (pointers, byte counts, sizes, base_p, growth_p) live in device memory, so the number of parts is
// not bounded by kernel-argument space (kJoinMaxParts bounds it).
//
// K15a join_check_kernel  one thread per (stream, output frame): the layout test of old_stream_kept for the frame's part,
//                         and the seek offsets of EVERY frame of every part: ordered, inside the body, each frame at least
//                         13 bytes and at least its own header plus the CRC-16, frame 0 at offset 0, its number field as
//                         long as its number's.  Runs before anything is copied; nothing later follows an offset it has
//                         not bounded.
// K15b join_size_kernel   one thread per stream: D_p(s) for every part and the new size (starts_scan_kernel follows).
// K15c join_kernel        one launch, `parts` workgroups of 256 per output stream (~64 KB of output each), no dependencies
//                         between workgroups, plain vector and byte stores.
#pragma once
#include "window_kernels.hpp"

namespace fa {

constexpr int kJoinBadLayout = 2;  // a stream of a part is not one this encoder wrote for that part's geometry
constexpr int kJoinBadTable = 8;   // a seek offset out of order or outside the body, a frame shorter than header + CRC-16
constexpr int64_t kJoinMaxParts = 1 << 16;

struct JoinPart {
    const uint8_t* old;  // the part's store
    int64_t old_bytes;
    const int64_t* old_starts;
    const int64_t* old_nbytes;
    int64_t size, nf, base, growth;  // N_p, nf_p, base_p, growth_p
};

struct JoinArgs {
    const JoinPart* part;   // [P], device
    int64_t* D;             // [P][n_stream] D_p(s) (written by the size kernel)
    const int64_t* starts;  // the new store
    int64_t* nbytes;
    uint8_t* out;
    int* err;  // kJoinBad*
    int64_t P, n_stream, size_new, nf_new, nchk;
    int32_t B, nch, parts, whole;
};

// what old_stream_kept reads of a splice's arguments
__device__ __forceinline__ SpliceArgs join_as_splice(const JoinArgs& a, const JoinPart& q) {
    SpliceArgs s;
    s.old = q.old; s.old_bytes = q.old_bytes; s.old_starts = q.old_starts; s.old_nbytes = q.old_nbytes;
    s.size_old = q.size; s.nf_old = q.nf; s.B = a.B; s.nch = a.nch;
    return s;
}

// the part that holds output frame g: the last one whose base is <= g (bases rise strictly: every part has a frame)
__device__ __forceinline__ int64_t join_find(const JoinArgs& a, int64_t g) {
    int64_t lo = 0, hi = a.P - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.part[mid].base <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// offset of frame k of a part's stream from its first frame (the body's end stands in for frame nf); h: the stream's first byte
__device__ __forceinline__ int64_t join_off(const JoinPart& q, const uint8_t* h, int64_t on, int64_t k) {
    return (k < q.nf) ? (int64_t)load_be64(h + 46 + 18 * k + 8) : on - stream_header_bytes(q.nf);
}

// ---- K15a ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void join_check_kernel(JoinArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_stream * a.nchk) return;
    const int64_t s = t / a.nchk, g = t - s * a.nchk;
    const JoinPart q = a.part[a.whole ? 0 : join_find(a, g)];
    const int64_t k = g - q.base;
    // the layout, before a seek point is read: every thread of the part's stream tests it, thread 0 reports it
    const SpliceArgs sa = join_as_splice(a, q);
    int64_t unused;
    if (!old_stream_kept(sa, s, q.nf, &unused)) {
        if (k == 0) atomicOr(a.err, kJoinBadLayout);
        return;
    }
    if (a.whole) return;  // copied as it is: no offset of its table is followed
    const uint8_t* h = q.old + q.old_starts[s];
    const int64_t on = q.old_nbytes[s], body = on - stream_header_bytes(q.nf);
    const int64_t off = join_off(q, h, on, k), end = join_off(q, h, on, k + 1);
    bool ok = off >= 0 && end <= body && off <= end && end - off >= kWindowMinFrame && (k != 0 || off == 0);
    if (ok) {
        // the frame holds its header and CRC-16, and its number field has the length of number k: the destination
        // offsets (append_growth) count on it
        int u;
        const int hl = window_header_len(h + stream_header_bytes(q.nf) + off, &u);
        ok = end - off >= (int64_t)hl + 2 && u == utf8_bytes((uint64_t)k);
    }
    if (!ok) atomicOr(a.err, kJoinBadTable);
}

// ---- K15b ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void join_size_kernel(JoinArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_stream) return;
    if (a.whole) {
        a.nbytes[s] = a.part[0].old_nbytes[s];
        return;
    }
    int64_t acc = 0;
    for (int64_t p = 0; p < a.P; ++p) {
        const JoinPart q = a.part[p];
        a.D[p * a.n_stream + s] = acc;
        acc += q.old_nbytes[s] - stream_header_bytes(q.nf) + q.growth;
    }
    a.nbytes[s] = stream_header_bytes(a.nf_new) + acc;
}

// ---- K15c ---------------------------------------------------------------------------------------------------------------
// grid: n_stream * parts workgroups of 256.  Workgroup (s, gp) writes its share of output stream s: (gp == 0) the fixed
// header; all of them share out part 0's seek points and body (verbatim) and the seek points of the later parts; their
// waves take the output frames g = nf_0 + 4 gp + wave, + 4 parts, ... of the later parts, find the source (p, k) in the
// base table and go through renumber_frame_wave with number g.  Every offset followed here was bounded by the check
// kernel for exactly these frames.
__global__ __launch_bounds__(256) void join_kernel(JoinArgs a) {
    const int64_t s = (int64_t)blockIdx.x / a.parts;
    const int gp = (int)((int64_t)blockIdx.x - s * a.parts);
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)gp * 256 + tid, nthr = (int64_t)a.parts * 256;
    uint8_t* const dst = a.out + a.starts[s];
    const JoinPart q0 = a.part[0];
    const uint8_t* const src0 = q0.old + q0.old_starts[s];
    const uint8_t* const end0 = q0.old + q0.old_bytes;
    const int64_t on0 = q0.old_nbytes[s];
    if (a.whole) {  // a single part: the stream as it is, its signature included
        copy_segment(dst, src0, on0, end0, t, nthr);
        return;
    }
    const int64_t hb = stream_header_bytes(a.nf_new), hb0 = stream_header_bytes(q0.nf);
    if (gp == 0)
        for (int i = tid; i < 46; i += 256) dst[i] = stream_header_byte(i, a.B, a.nch, a.size_new, a.nf_new);  // (no MD5: other samples)
    // part 0 keeps its numbers and offsets: its points and its frames as they are
    copy_segment(dst + 46, src0 + 46, 18 * q0.nf, end0, t, nthr);
    copy_segment(dst + hb, src0 + hb0, on0 - hb0, end0, t, nthr);
    // the later parts' seek points: sample, offset, samples (big-endian)
    for (int64_t g = q0.nf + t; g < a.nf_new; g += nthr) {
        const int64_t p = join_find(a, g);
        const JoinPart q = a.part[p];
        const int64_t k = g - q.base;
        const uint8_t* sp = q.old + q.old_starts[s] + 46 + 18 * k;
        uint8_t* pt = dst + 46 + 18 * g;
        store_be64(pt, (uint64_t)g * (uint64_t)a.B);
        store_be64(pt + 8, (uint64_t)(a.D[p * a.n_stream + s] + (int64_t)load_be64(sp + 8) + append_growth(q.base, k)));
        pt[16] = sp[16];
        pt[17] = sp[17];
    }
    // the later parts' frames, one per wave at a time
    const int wave = tid >> 6, lane = tid & 63;
    for (int64_t g = q0.nf + (int64_t)gp * 4 + wave; g < a.nf_new; g += (int64_t)a.parts * 4) {
        const int64_t p = join_find(a, g);
        const JoinPart q = a.part[p];
        const int64_t k = g - q.base;
        const uint8_t* h = q.old + q.old_starts[s];
        const int64_t on = q.old_nbytes[s];
        const int64_t off = join_off(q, h, on, k), end = join_off(q, h, on, k + 1);
        renumber_frame_wave(dst + hb + a.D[p * a.n_stream + s] + off + append_growth(q.base, k), h + stream_header_bytes(q.nf) + off, end - off,
                            (uint64_t)g, q.old + q.old_bytes, lane);
    }
}

}  // namespace fa
