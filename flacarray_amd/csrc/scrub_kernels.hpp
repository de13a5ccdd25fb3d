// scrub_kernels.hpp -- the damage map of a store and the fill of the salvage decode, for gfx950 (wave64).
//
// A store whose bytes were damaged has no way through K6 / K7: one bad stream header, seek point or frame fails the
// whole call (the error word is one per call).  The kernels here answer per (stream, frame) instead, from nothing but
// the store, and never report through an error word:
//
//   scrub_streams_kernel  one thread per stream: the tolerant twin of parse_streams_kernel -- a StreamMeta for every
//                         stream that can be located (first_frame = -1 for every other) and a per-stream flag
//   scrub_table_kernel    one thread per (stream, frame): the tolerant frame table, -1 where seek point f is unusable
//   frame_status_kernel   one wavefront per (stream, frame): locates the frame, checks its header (frame number and
//                         block size included) and its CRC-16, writes one status byte
//   fill_ranges_kernel    writes a fill value over a table of output ranges (what the salvage decode does not decode)
//
// The status rule (README "Damage", DESIGN "Damage map and salvage"; tests/scrub_model.py restates it over bytes):
//   stream located   0 <= start, 0 <= nbytes, start + nbytes <= blob size; "fLaC"; the metadata chain parses inside
//                    nbytes; STREAMINFO min == max block size == B with nch channels; a SEEKTABLE of exactly nf points
//   frame located    seek point f carries sample number f B; begin = first_frame + offset_f; end = the begin of frame
//                    f + 1 found the same way (the stream's end for the last frame); first_frame <= begin,
//                    begin + 8 <= end, end <= stream end.  Otherwise FRAME_UNLOCATED and nothing of the frame is read.
//   located frames   FRAME_HEADER: the header K7 would reject, a frame number other than f, or a block size other than
//                    min(B, N - f B); FRAME_CRC16: the CRC-16 over [begin, end - 2) differs from the two stored bytes.
// Every offset is checked against the stream's end before a byte behind it is read.
#pragma once
#include "decode_kernels.hpp"
#include "encode_fused.hpp"

namespace fa {

constexpr int kFrameOk = 0;
constexpr int kFrameUnlocated = 1;
constexpr int kFrameHeader = 2;
constexpr int kFrameCrc16 = 4;

__global__ __launch_bounds__(256) void scrub_streams_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ starts,
                                                            const int64_t* __restrict__ nbytes, int64_t n_stream, int64_t nf,
                                                            int64_t blob_bytes, int32_t B, int32_t nch,
                                                            StreamMeta* __restrict__ meta, uint8_t* __restrict__ located) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_stream) return;
    const int64_t st0 = starts[s];
    const int64_t nb = nbytes[s];
    StreamMeta m;
    m.first_frame = -1; m.seek_abs = -1; m.end_abs = 0; m.npoints = 0; m.B = 0; m.bps = 0; m.flags = 0; m.channels = 0;
    // nothing of the stream is touched before its extent is known to lie inside the blob
    if (st0 < 0 || nb < 0 || st0 > blob_bytes || nb > blob_bytes - st0) {
        meta[s] = m;
        located[s] = 0;
        return;
    }
    const uint8_t* p = blob + st0;
    m.end_abs = st0 + nb;
    bool ok = nb >= 4 && p[0] == 'f' && p[1] == 'L' && p[2] == 'a' && p[3] == 'C';
    bool have_info = false;
    int minb = 0;
    int64_t off = 4;
    while (ok) {
        if (off + 4 > nb) { ok = false; break; }
        const int last = p[off] >> 7, type = p[off] & 0x7f;
        const int64_t len = ((int64_t)p[off + 1] << 16) | ((int64_t)p[off + 2] << 8) | p[off + 3];
        off += 4;
        if (off + len > nb) { ok = false; break; }
        if (type == 0 && len >= 34) {
            minb = (p[off] << 8) | p[off + 1];
            m.B = (p[off + 2] << 8) | p[off + 3];
            m.bps = (((p[off + 12] & 1) << 4) | (p[off + 13] >> 4)) + 1;
            m.channels = ((p[off + 12] >> 1) & 7) + 1;
            have_info = true;
        } else if (type == 3) {
            m.seek_abs = st0 + off;
            m.npoints = (int32_t)(len / 18);
        }
        off += len;
        if (last) break;
    }
    ok = ok && have_info && minb == B && m.B == B && m.channels == nch && m.seek_abs >= 0 && (int64_t)m.npoints == nf;
    if (ok) {
        m.first_frame = st0 + off;
        m.flags = 1;
    }
    meta[s] = m;
    located[s] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void scrub_table_kernel(const uint8_t* __restrict__ blob, const StreamMeta* __restrict__ meta,
                                                          const uint8_t* __restrict__ located, int64_t n_stream, int64_t nf, int32_t B,
                                                          int64_t* __restrict__ ftab) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_stream * nf) return;
    const int64_t s = t / nf, f = t - s * nf;
    if (!located[s]) { ftab[t] = -1; return; }
    const StreamMeta m = meta[s];
    const uint8_t* sp = blob + m.seek_abs + 18 * f;  // (the table lies inside the stream: scrub_streams_kernel)
    const uint64_t sn = load_be64(sp), off = load_be64(sp + 8);
    // an offset that leaves the stream gives no begin: first_frame + off is never formed for it
    const bool usable = sn == (uint64_t)f * (uint64_t)B && off <= (uint64_t)(m.end_abs - m.first_frame);
    ftab[t] = usable ? m.first_frame + (int64_t)off : -1;
}

// byte i (0..15) of a header held as two big-endian words
__device__ __forceinline__ uint32_t scrub_hdr_byte(uint64_t hi, uint64_t lo, int i) {
    return (uint32_t)(((i < 8) ? (hi >> (56 - 8 * i)) : (lo >> (120 - 8 * i))) & 0xFFu);
}

// the header of frame f as `avail` >= 8 bytes hold it (RFC 9639 9.1): what K7 rejects, plus the frame number and the
// coded block size; a header longer than the frame counts as bad
__device__ __forceinline__ bool scrub_header_ok(uint64_t hi, uint64_t lo, int avail, int nch, int64_t f, int expect_bs) {
    const uint32_t b0 = scrub_hdr_byte(hi, lo, 0), b1 = scrub_hdr_byte(hi, lo, 1), b2 = scrub_hdr_byte(hi, lo, 2), b3 = scrub_hdr_byte(hi, lo, 3);
    if (b0 != 0xFFu || b1 != 0xF8u) return false;  // sync, reserved 0, fixed blocksize
    const int bsc = (int)(b2 >> 4), src = (int)(b2 & 15), ch = (int)(b3 >> 4), ssc = (int)((b3 >> 1) & 7);
    if (bsc == 0 || src == 15 || ssc == 3 || !channel_code_ok(ch, nch) || (b3 & 1)) return false;
    const uint32_t u0 = scrub_hdr_byte(hi, lo, 4);
    int extra = 0;
    uint64_t num = u0;
    if (u0 & 0x80) {
        int mbit = 0x40;
        while ((u0 & mbit) && extra < 7) { extra++; mbit >>= 1; }
        if (extra == 0 || extra > 6) return false;
        num = u0 & (uint32_t)(mbit - 1);
    }
    const int n = 5 + extra + (bsc == 6 ? 1 : bsc == 7 ? 2 : 0) + (src == 12 ? 1 : (src == 13 || src == 14) ? 2 : 0);  // bytes under the CRC-8
    if (n + 1 > avail || n + 1 > 16) return false;
    int at = 5;
    for (int i = 0; i < extra; ++i) {
        const uint32_t c = scrub_hdr_byte(hi, lo, at++);
        if ((c & 0xC0u) != 0x80u) return false;
        num = (num << 6) | (c & 0x3Fu);
    }
    if (num != (uint64_t)f) return false;
    int bs;
    if (bsc == 1) bs = 192;
    else if (bsc <= 5) bs = 576 << (bsc - 2);
    else if (bsc == 6) bs = (int)scrub_hdr_byte(hi, lo, at) + 1;
    else if (bsc == 7) bs = (int)((scrub_hdr_byte(hi, lo, at) << 8) | scrub_hdr_byte(hi, lo, at + 1)) + 1;
    else bs = 256 << (bsc - 8);
    if (bs != expect_bs) return false;
    uint8_t c8 = 0;
    for (int i = 0; i < n; ++i) c8 = crc8_byte(c8, (uint8_t)scrub_hdr_byte(hi, lo, i));
    return c8 == (uint8_t)scrub_hdr_byte(hi, lo, n);
}

// One wavefront per (stream, frame) of the whole store, four per workgroup.  The CRC-16 fold is verify_crc16_kernel's
// (verify_kernels.hpp), kept apart from it: K9 has to stay inside the 48 registers that fit beside two waves of K7, and
// this kernel carries the header words and the status through the fold.
__global__ __launch_bounds__(256) void frame_status_kernel(const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                                           const StreamMeta* __restrict__ meta, const int64_t* __restrict__ ftab,
                                                           int64_t n_stream, int64_t nf, int32_t B, int64_t stream_size, int32_t nch,
                                                           const uint16_t* __restrict__ crc_tab, uint8_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint16_t crc_s[kFCrcSlice];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kFCrcSlice / 2; i += 256) reinterpret_cast<uint32_t*>(crc_s)[i] = reinterpret_cast<const uint32_t*>(crc_tab)[i];
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 4 + (tid >> 6);
    if (t >= n_stream * nf) return;
    const int64_t s = t / nf, f = t - s * nf;
    const StreamMeta m = meta[s];
    const int64_t start = ftab[t];
    const int64_t end = (m.first_frame < 0) ? -1 : (f + 1 < nf) ? ftab[t + 1] : m.end_abs;
    // m.end_abs <= blob_bytes (scrub_streams_kernel), start >= m.first_frame (scrub_table_kernel): every byte of
    // [start, end) is a byte of the stream
    if (m.first_frame < 0 || start < 0 || end < 0 || start + 8 > end || end > m.end_abs || end > blob_bytes) {
        if (lane == 0) status[t] = (uint8_t)kFrameUnlocated;
        return;
    }
    const uint8_t* p = blob + start;
    // the header's bytes (at most 16), loaded before the fold and looked at after it
    uint64_t hdr_hi = 0, hdr_lo = 0;
    const int avail = (end - start < 16) ? (int)(end - start) : 16;
    if (lane == 0) {
        if (avail == 16) {
            uint64_t r0, r1;
            __builtin_memcpy(&r0, p, 8);  // (any byte alignment)
            __builtin_memcpy(&r1, p + 8, 8);
            hdr_hi = __builtin_bswap64(r0);
            hdr_lo = __builtin_bswap64(r1);
        } else {
            for (int i = 0; i < avail; ++i) {
                if (i < 8) hdr_hi |= (uint64_t)p[i] << (56 - 8 * i);
                else hdr_lo |= (uint64_t)p[i] << (120 - 8 * i);
            }
        }
    }
    const int64_t L = end - start - 2;  // bytes covered by the CRC (64-bit: a damaged table may give any extent inside the stream)
    uint32_t crc_t = 0;
    int64_t last_end = 0;
    bool any = false;
    // eight 256-byte stripes per lane in flight, whole 2048-byte trips without masks, the tail word by word
    constexpr int kBatch = 8;
    const int64_t Lin = L & ~(int64_t)3;  // whole words under the CRC: all inside the blob, end <= blob_bytes
    int64_t base = 0;
    for (; base + 256 * kBatch <= Lin; base += 256 * kBatch) {
        const uint8_t* q = p + base + 4 * lane;
        uint32_t raw[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) __builtin_memcpy(&raw[k], q + 256 * k, 4);  // (any byte alignment)
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const uint32_t w = __builtin_bswap32(raw[k]) ^ (crc_t << 16);
            crc_t = (uint32_t)crc_s[w >> 24] ^ (uint32_t)crc_s[256 + ((w >> 16) & 255u)] ^ (uint32_t)crc_s[512 + ((w >> 8) & 255u)] ^
                    (uint32_t)crc_s[768 + (w & 255u)];
        }
        last_end = base + 256 * (kBatch - 1) + 4 * lane + 4;
        any = true;
    }
    for (int64_t o = base + 4 * lane; o < L; o += 256) {
        uint32_t w;
        if (start + o + 4 <= blob_bytes) {
            uint32_t raw;
            __builtin_memcpy(&raw, p + o, 4);
            w = __builtin_bswap32(raw);
        } else {  // the last bytes of the blob: byte by byte
            w = 0;
            for (int b2 = 0; b2 < 4 && start + o + b2 < blob_bytes; ++b2) w |= (uint32_t)p[o + b2] << (24 - 8 * b2);
        }
        if (o + 4 > L) w &= ~0u << (8u * (uint32_t)(4 - (L - o)));  // bytes at and after L (the CRC itself) do not count
        w ^= crc_t << 16;
        crc_t = (uint32_t)crc_s[w >> 24] ^ (uint32_t)crc_s[256 + ((w >> 16) & 255u)] ^ (uint32_t)crc_s[512 + ((w >> 8) & 255u)] ^
                (uint32_t)crc_s[768 + (w & 255u)];
        last_end = o + 4;
        any = true;
    }
    // x^(8k) combine of the lanes' states, xor butterfly (as K9)
    uint32_t contrib = 0;
    if (any) contrib = crc16_mulmod((uint16_t)crc_t, crc_tab[kFCrcSlice + (int)(L - last_end) + 3]);
    contrib ^= (uint32_t)xchg_i32<0>((int)contrib);
    contrib ^= (uint32_t)xchg_i32<1>((int)contrib);
    contrib ^= (uint32_t)xchg_i32<2>((int)contrib);
    contrib ^= (uint32_t)xchg_i32<3>((int)contrib);
    contrib ^= (uint32_t)xchg_i32<4>((int)contrib);
    const uint32_t crc = ((uint32_t)__builtin_amdgcn_readlane((int)contrib, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)contrib, 32)) & 0xFFFFu;
    if (lane == 0) {
        const uint32_t stored = ((uint32_t)p[L] << 8) | (uint32_t)p[L + 1];
        int64_t expect = stream_size - f * (int64_t)B;
        if (expect > B) expect = B;
        int st = kFrameOk;
        if (!scrub_header_ok(hdr_hi, hdr_lo, avail, nch, f, (int)expect)) st |= kFrameHeader;
        if (crc != stored) st |= kFrameCrc16;
        status[t] = (uint8_t)st;
    }
}

// One workgroup per range of the table, its four wavefronts taking the range's 2048-element pieces in turn: lane l of a
// piece's wave writes elements l, l + 64, ... of it, element by element -- range starts, lengths and the base pointer
// have any alignment the type allows, and nothing outside [off, off + count) is written.
template <typename T>
__global__ __launch_bounds__(256) void fill_ranges_kernel(T* __restrict__ out, int64_t n_ranges, const int64_t* __restrict__ off,
                                                          const int64_t* __restrict__ count, T fill) {
    constexpr int64_t kPiece = 2048;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = blockIdx.x; r < n_ranges; r += gridDim.x) {
        const int64_t o = off[r], n = count[r];
        if (o < 0 || n <= 0) continue;
        for (int64_t p0 = (int64_t)wave * kPiece; p0 < n; p0 += 4 * kPiece) {
            const int64_t len = (n - p0 < kPiece) ? n - p0 : kPiece;
            T* const q = out + o + p0;
            for (int64_t i = lane; i < len; i += 64) q[i] = fill;
        }
    }
}

}  // namespace fa
