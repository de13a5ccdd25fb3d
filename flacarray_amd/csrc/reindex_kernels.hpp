// reindex_kernels.hpp -- K13, FlacArray.reindex on gfx950 (wave64): copy every stream of a store into this library's
// own layout, whatever metadata it came with.
//
// A stream libFLAC wrote is "fLaC", STREAMINFO, VORBIS_COMMENT and the frames: it has no seek point per frame, so the
// splice (K10) refuses it and the damage map (K12) reports every frame FRAME_UNLOCATED.  K6 already locates its frames
// (sync scan or walk); what is missing is writing that table back.  With the StreamMeta[S] / ftab[S][nf] tables of K6
// at hand, the output stream is exactly
//     bytes 0-3        "fLaC"
//     bytes 4-7        00 00 00 22: STREAMINFO, not last (whatever the source's last-flag was)
//     bytes 8-41       the source's 34 STREAMINFO bytes verbatim (block and frame sizes, rate / channels / bps / total,
//                      MD5: a signed stream stays signed)
//     bytes 42-45      83, then 18 nf as 24 bits big-endian: the SEEKTABLE, last
//     46 + 18 f        seek point f: sample number f B (u64), offset ftab[f] - ftab[0] (u64), min(B, N - f B) (u16)
//     46 + 18 nf ...   the source bytes [first_frame, end_abs) verbatim
// No sample is decoded and no frame re-encoded.  Every other metadata block of the source (VORBIS_COMMENT, APPLICATION,
// PADDING, a sparse or placeholder SEEKTABLE) is dropped: this layout has no room for it.  A stream that already has this
// layout comes out byte-identical.
//
// K13a reindex_check_kernel  one thread per (stream, frame).  K6 does not bound the offsets it takes from a complete
//                            SEEKTABLE (build_frame_table_kernel relies on K7's own bounds, and here no K7 follows):
//                            the table must start at first_frame, increase strictly and leave 8 bytes for the last
//                            frame inside the stream, and the first metadata block must be a 34-byte STREAMINFO at
//                            byte 4 -- the copy takes bytes 8-41 for it.  The last frame must carry number nf - 1 and
//                            N - (nf - 1) B samples: the walk counts frames without reading their numbers, so this
//                            is what refuses a stream_size that is not the store's.
// K13b reindex_size_kernel   one thread per stream: 46 + 18 nf + (end_abs - first_frame); starts_scan_kernel follows.
// K13c reindex_kernel        `parts` workgroups of 256 per stream (~64 KB of output each, the splice's rule), no
//                            dependencies between workgroups, plain vector and byte stores; the seek points are shared
//                            out over all parts of a stream (a 65 600-frame stream has 1.2 MB of them), the body is
//                            K10's copy_segment.
#pragma once
#include "decode_kernels.hpp"
#include "splice_kernels.hpp"  // (copy_segment, store_be64)

namespace fa {

constexpr int kReindexBadTable = 1;
constexpr int kReindexBadHeader = 2;
constexpr int kReindexBadSize = 4;
constexpr int64_t kReindexMaxFrames = 0xFFFFFF / 18;  // 932 067: the SEEKTABLE's length field has 24 bits

struct ReindexArgs {
    const uint8_t* src;  // the caller's store (16-byte aligned), its index, and K6's tables of it
    int64_t src_bytes;
    const int64_t* src_starts;
    const StreamMeta* meta;
    const int64_t* ftab;
    const int64_t* starts;  // the new store
    int64_t* nbytes;
    uint8_t* out;
    int* err;  // kReindexBadTable | kReindexBadHeader | kReindexBadSize
    int64_t n_stream, nf, stream_size;
    int32_t B, parts;
};

// The header at p (avail >= 8 bytes of its stream) is a fixed-blocksize frame header that carries frame number `num` and
// codes `bs` samples.  (Number and block size only: the CRC-8 and the rest of the header are K12's to judge.)
__device__ __forceinline__ bool reindex_frame_is(const uint8_t* p, int64_t avail, uint64_t num, int bs) {
    if (p[0] != 0xFF || p[1] != 0xF8) return false;
    const int bsc = p[2] >> 4;
    const uint32_t u0 = p[4];
    int extra = 0;
    uint64_t got = u0;
    if (u0 & 0x80) {
        int mbit = 0x40;
        while ((u0 & mbit) && extra < 7) { extra++; mbit >>= 1; }
        if (extra == 0 || extra > 5) return false;
        got = u0 & (uint32_t)(mbit - 1);
    }
    const int at = 5 + extra;
    if (at + (bsc == 6 ? 1 : bsc == 7 ? 2 : 0) > avail) return false;
    for (int i = 0; i < extra; ++i) {
        const uint32_t c = p[5 + i];
        if ((c & 0xC0) != 0x80) return false;
        got = (got << 6) | (c & 0x3F);
    }
    int coded;
    if (bsc == 0) return false;
    else if (bsc == 1) coded = 192;
    else if (bsc <= 5) coded = 576 << (bsc - 2);
    else if (bsc == 6) coded = (int)p[at] + 1;
    else if (bsc == 7) coded = (((int)p[at] << 8) | (int)p[at + 1]) + 1;
    else coded = 256 << (bsc - 8);
    return got == num && coded == bs;
}

// ---- K13a -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reindex_check_kernel(ReindexArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_stream * a.nf) return;
    const int64_t s = t / a.nf, f = t - s * a.nf;
    const StreamMeta m = a.meta[s];
    const int64_t st0 = a.src_starts[s];
    // what K6 accepted: 0 <= start, 42 <= nbytes, end_abs <= src_bytes, start + 42 <= first_frame <= end_abs -- tested
    // again, nothing of the stream is read before it holds
    if (st0 < 0 || m.first_frame < st0 + 42 || m.first_frame > m.end_abs || m.end_abs > a.src_bytes) {
        atomicOr(a.err, kReindexBadHeader);
        return;
    }
    if (f == 0) {
        const uint8_t* h = a.src + st0;
        if ((h[4] & 0x7F) != 0 || h[5] != 0 || h[6] != 0 || h[7] != 34) atomicOr(a.err, kReindexBadHeader);
    }
    const int64_t v = a.ftab[t];
    bool ok = (f == 0) ? (v == m.first_frame) : (v > m.first_frame);
    if (f + 1 < a.nf) ok = ok && v < a.ftab[t + 1];
    else ok = ok && v <= m.end_abs - 8;
    if (!ok) atomicOr(a.err, kReindexBadTable);
    // the last frame is frame nf - 1 of N - (nf - 1) B samples: what ties the call's stream_size to the store (the walk
    // follows nf frames without looking at their numbers, so a stream_size too small would pass everything above)
    if (ok && f + 1 == a.nf &&
        !reindex_frame_is(a.src + v, m.end_abs - v, (uint64_t)f, (int)(a.stream_size - f * (int64_t)a.B)))
        atomicOr(a.err, kReindexBadSize);
}

// ---- K13b -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reindex_size_kernel(ReindexArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_stream) return;
    const StreamMeta m = a.meta[s];
    const int64_t body = (m.first_frame >= 0 && m.first_frame <= m.end_abs) ? m.end_abs - m.first_frame : 0;
    a.nbytes[s] = stream_header_bytes(a.nf) + body;
}

// ---- K13c: the copy (after the check: every ftab entry lies in [first_frame, end_abs - 8], end_abs <= src_bytes) ------
__global__ __launch_bounds__(256) void reindex_kernel(ReindexArgs a) {
    const int64_t s = (int64_t)blockIdx.x / a.parts;
    const int p = (int)((int64_t)blockIdx.x - s * a.parts);
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)p * 256 + tid, nthr = (int64_t)a.parts * 256;
    const StreamMeta m = a.meta[s];
    uint8_t* const dst = a.out + a.starts[s];
    if (p == 0 && tid < 46) {
        const uint32_t stl = 18u * (uint32_t)a.nf;
        uint8_t b;
        if (tid < 4) b = (uint8_t)(0x43614C66u >> (8 * tid));  // "fLaC"
        else if (tid < 8) b = (tid == 7) ? 34 : 0;
        else if (tid < 42) b = a.src[a.src_starts[s] + tid];
        else if (tid == 42) b = 0x83;
        else b = (uint8_t)(stl >> (8 * (45 - tid)));
        dst[tid] = b;
    }
    const int64_t* const ft = a.ftab + s * a.nf;
    for (int64_t f = t; f < a.nf; f += nthr) {
        uint8_t* pt = dst + 46 + 18 * f;
        int64_t cnt = a.stream_size - f * (int64_t)a.B;
        if (cnt > a.B) cnt = a.B;
        store_be64(pt, (uint64_t)f * (uint64_t)a.B);
        store_be64(pt + 8, (uint64_t)(ft[f] - m.first_frame));
        pt[16] = (uint8_t)(cnt >> 8);
        pt[17] = (uint8_t)cnt;
    }
    copy_segment(dst + stream_header_bytes(a.nf), a.src + m.first_frame, m.end_abs - m.first_frame, a.src + a.src_bytes, t, nthr);
}

}  // namespace fa
