// md5_kernels.hpp -- the STREAMINFO MD5 signature (RFC 1321) of many streams at once on gfx950.
//
// K10 md5_rows_kernel     : MD5 of every row of an int32 / int64 image (or a float32 / float64 image quantised where it
//                           is loaded), ONE LANE PER STREAM, resumable through a per-stream chaining state
// K11 md5_classify_kernel : per stream, what a check can say before anything is decoded (unsigned / not checkable)
//     md5_compare_kernel  : computed digest against the sixteen bytes in STREAMINFO
//     sign_check_kernel / sign_streams_kernel : write digests into bytes [26, 42) of every stream
//
// What libFLAC hashes (FLAC__MD5Accumulate) is the interleaved samples, little-endian, ceil(bps / 8) bytes each.  For the
// streams of this library -- 32 bits per sample, one channel (int32) or two (int64: channel 0 = low word, channel 1 = high
// word) -- that is exactly the bytes of the integer row, so the kernel hashes dwords and never looks at a sample width.
//
// MD5 is a serial chain inside a stream (64 dependent steps per 64-byte block); the parallelism is across streams.  A lane
// that read its own row directly would touch 64 cache lines per load instruction, so a wave (= a block: 64 streams) fetches
// kMd5TileBlocks consecutive 64-byte blocks of each of its streams with coalesced loads (16 bytes per lane where the rows
// are 16-byte aligned) into registers, moves them into an LDS tile of pitch 65 dwords -- lane l reading word w of its own
// row hits bank (l + w) mod 32 within its group of 32 lanes: no conflicts -- and hashes out of the tile.  The loads of tile t + 1 are issued before tile
// t is hashed and land in registers while the chain runs (64 VGPRs): with n_stream / 64 waves on the machine occupancy
// hides nothing, that prefetch does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "quantize_kernels.hpp"

namespace fa {

constexpr int kMd5TileBlocks = 4;                       // 64-byte blocks of every stream per tile
constexpr int kMd5TileDwords = 16 * kMd5TileBlocks;     // 64 dwords = 256 bytes of a row
constexpr int kMd5Pitch = kMd5TileDwords + 1;           // odd in dwords
static_assert(kMd5TileDwords == 64, "the load mapping assumes one 256-byte row segment per 64 / 32 / 16 lanes");

// one 64-byte block; m[] under constant indices only (fully unrolled), so the message stays in registers
__device__ __forceinline__ void md5_block(uint32_t (&h)[4], const uint32_t (&m)[16]) {
    constexpr uint32_t K[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu,
        0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau,
        0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u,
        0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u,
        0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u,
        0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        int g;
        if (i < 16) { f = d ^ (b & (c ^ d)); g = i; }
        else if (i < 32) { f = c ^ (d & (b ^ c)); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        const uint32_t t = a + f + K[i] + m[g];
        a = d;
        d = c;
        c = b;
        b = b + __builtin_rotateleft32(t, S[(i >> 4) * 4 + (i & 3)]);
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

// What a lane holds of the next tile: 64 dwords of raw input, as load units of U dwords.
template <int U> struct Md5Unit;
template <> struct Md5Unit<1> { using type = uint32_t; };
template <> struct Md5Unit<2> { using type = uint2; };
template <> struct Md5Unit<4> { using type = uint4; };

// raw input dwords -> the integer's dwords (identity for integer rows); nd: how many of w[] are inside the row
template <int KIND>
__device__ __forceinline__ void md5_convert(uint32_t (&w)[4], int nd, float off32, float gain32, double off64, double gain64, bool& nan) {
    if (KIND == 2) {  // float32 -> int32
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nd) {
                const float x = __uint_as_float(w[e]);
                nan = nan || (x != x);
                w[e] = (uint32_t)quantise_f32(x, off32, gain32);
            }
    } else if (KIND == 3) {  // float64 -> int64 (low word first)
#pragma unroll
        for (int e = 0; e < 4; e += 2)
            if (e < nd) {
                const double x = __hiloint2double((int)w[e + 1], (int)w[e]);
                nan = nan || (x != x);
                const int64_t q = quantise_f64(x, off64, gain64);
                w[e] = (uint32_t)(uint64_t)q;
                w[e + 1] = (uint32_t)((uint64_t)q >> 32);
            }
    }
}

// KIND 0: int32 rows, 1: int64 rows, 2: float32 rows + offsets / gains, 3: float64 rows + offsets / gains.
// U: dwords per load (4 needs every row 16-byte aligned: base and stride; 2 is the element of the 8-byte kinds).
// data: rows of `nd` dwords, `stride_d` dwords apart.  n_before_bytes: bytes of every stream hashed by earlier calls (a
// multiple of 64).  !final: nd is a multiple of 16, state_out receives the chaining state.  final: the padding and the bit
// length of (n_before_bytes + 4 nd) are hashed, digest receives 16 bytes per stream.  state_in is read only when
// something was hashed before.  One wave per block, 64 streams per block; no waiting between waves, no atomics but the
// NaN flag.
template <int KIND, int U>
FA_GLOBAL __global__ __launch_bounds__(64) void md5_rows_kernel(const uint32_t* __restrict__ data, int64_t n_stream, int64_t nd, int64_t stride_d,
                                                                const void* __restrict__ offsets, const void* __restrict__ gains,
                                                                const uint32_t* state_in, uint64_t n_before_bytes, int final,
                                                                uint32_t* state_out, uint32_t* __restrict__ digest,
                                                                int* __restrict__ flags) {
    constexpr int LPS = kMd5TileDwords / U;  // lanes that share one stream's 256-byte segment
    constexpr int SPI = 64 / LPS;            // streams per load instruction
    constexpr int NL = 64 / SPI;             // load instructions per tile
    using unit_t = typename Md5Unit<U>::type;
    __shared__ uint32_t tile[64 * kMd5Pitch];
    // float kinds: the 64 streams' offsets and gains, fetched once (a load per tile would sit in front of every deposit)
    __shared__ double par[KIND >= 2 ? 128 : 1];
    const int lane = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * 64;
    const int64_t my = s0 + lane;
    const int sub = lane / LPS;           // which of the SPI streams of a load instruction this lane fetches for
    const int col = (lane % LPS) * U;     // dword inside the segment

    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    if (n_before_bytes != 0 && my < n_stream) {
        const uint4 v = reinterpret_cast<const uint4*>(state_in)[my];
        h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
    }

    if (KIND >= 2) {
        const int64_t s = my < n_stream ? my : n_stream - 1;
        if (KIND == 2) {
            reinterpret_cast<float*>(par)[lane] = reinterpret_cast<const float*>(offsets)[s];
            reinterpret_cast<float*>(par)[64 + lane] = reinterpret_cast<const float*>(gains)[s];
        } else {
            par[lane] = reinterpret_cast<const double*>(offsets)[s];
            par[64 + lane] = reinterpret_cast<const double*>(gains)[s];
        }
    }  // (the first deposit is behind a barrier)
    const int64_t rounds = (nd + kMd5TileDwords - 1) / kMd5TileDwords;
    const int64_t blocks = nd / 16;
    unit_t pre[NL];
    bool nan = false;

    // (lanes of streams past the end fetch the last stream again: no divergence, nothing stored for them)
    const uint32_t* src[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        int64_t s = s0 + i * SPI + sub;
        if (s >= n_stream) s = n_stream - 1;
        src[i] = data + s * stride_d + col;
    }
    auto fetch = [&](int64_t t) {
        const int64_t c0 = t * kMd5TileDwords;
        if (c0 + kMd5TileDwords <= nd) {  // (uniform) a whole tile: nothing but the loads
#pragma unroll
            for (int i = 0; i < NL; ++i) pre[i] = *reinterpret_cast<const unit_t*>(src[i] + c0);
            return;
        }
        const int64_t c = c0 + col;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const uint32_t* p = src[i] + c0;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < U; ++e)
                if (c + e < nd) w[e] = p[e];
            if (U == 1) *reinterpret_cast<uint32_t*>(&pre[i]) = w[0];
            if (U == 2) *reinterpret_cast<uint2*>(&pre[i]) = make_uint2(w[0], w[1]);
            if (U == 4) *reinterpret_cast<uint4*>(&pre[i]) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    // (whole: every dword of the tile is inside the row -- the float kinds then convert without a bounds test per value)
    auto deposit_as = [&](int64_t t, auto whole) {
        const int64_t c = t * kMd5TileDwords + col;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int r = i * SPI + sub;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (U == 1) w[0] = *reinterpret_cast<const uint32_t*>(&pre[i]);
            if (U == 2) { const uint2 v = *reinterpret_cast<const uint2*>(&pre[i]); w[0] = v.x; w[1] = v.y; }
            if (U == 4) { const uint4 v = *reinterpret_cast<const uint4*>(&pre[i]); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
            if (KIND >= 2) {
                const int64_t left = nd - c;
                const int valid = (decltype(whole)::value || left >= U) ? U : (left > 0 ? (int)left : 0);
                float o32 = 0.f, g32 = 0.f;
                double o64 = 0., g64 = 0.;
                if (KIND == 2) { o32 = reinterpret_cast<const float*>(par)[r]; g32 = reinterpret_cast<const float*>(par)[64 + r]; }
                if (KIND == 3) { o64 = par[r]; g64 = par[64 + r]; }
                md5_convert<KIND>(w, valid, o32, g32, o64, g64, nan);
            }
#pragma unroll
            for (int e = 0; e < U; ++e) tile[r * kMd5Pitch + col + e] = w[e];
        }
    };
    auto deposit = [&](int64_t t) {
        if (KIND >= 2 && (t + 1) * kMd5TileDwords <= nd) deposit_as(t, std::true_type{});
        else deposit_as(t, std::false_type{});
    };

    const uint32_t* row = tile + lane * kMd5Pitch;
    if (rounds > 0) fetch(0);
    for (int64_t t = 0; t < rounds; ++t) {
        __syncthreads();  // the tile is free: every lane has hashed what it held
        deposit(t);
        __syncthreads();
        if (t + 1 < rounds) fetch(t + 1);  // in flight while the chain below runs
        int64_t kb = blocks - t * kMd5TileBlocks;
        if (kb > kMd5TileBlocks) kb = kMd5TileBlocks;
        for (int b = 0; b < (int)kb; ++b) {
            uint32_t m[16];
#pragma unroll
            for (int w = 0; w < 16; ++w) m[w] = row[b * 16 + w];
            md5_block(h, m);
        }
    }

    if (final) {
        // the unfinished block (rem dwords, zeros behind them: the fetch fills with zeros) is in the last tile; the 0x80 lands
        // on a dword boundary because the message is dwords.  Every lane touches its own row of the tile only.
        uint32_t* mine = tile + lane * kMd5Pitch;
        const int rem = (int)(nd & 15);
        int base = 0;
        if (rem == 0) {
            for (int w = 0; w < 16; ++w) mine[w] = 0u;
        } else {
            base = (int)(blocks % kMd5TileBlocks) * 16;
        }
        mine[base + rem] = 0x80u;
        uint32_t m[16];
        if (rem >= 14) {
#pragma unroll
            for (int w = 0; w < 16; ++w) m[w] = mine[base + w];
            md5_block(h, m);
            for (int w = 0; w < 16; ++w) mine[base + w] = 0u;
        }
        const uint64_t bits = (n_before_bytes + (uint64_t)nd * 4u) * 8u;
        mine[base + 14] = (uint32_t)bits;
        mine[base + 15] = (uint32_t)(bits >> 32);
#pragma unroll
        for (int w = 0; w < 16; ++w) m[w] = mine[base + w];
        md5_block(h, m);
        if (my < n_stream) reinterpret_cast<uint4*>(digest)[my] = make_uint4(h[0], h[1], h[2], h[3]);
    } else if (my < n_stream) {
        reinterpret_cast<uint4*>(state_out)[my] = make_uint4(h[0], h[1], h[2], h[3]);
    }
    if (KIND >= 2 && __any(nan) && lane == 0) atomicOr(flags, 1);
}

// ---- STREAMINFO: "fLaC", block header (type 0, length 34), then at +18 sample rate (20 bits), channels - 1 (3),
// bits per sample - 1 (5), total samples (36), and the MD5 at +26 ----
constexpr int kMd5Offset = 26;
constexpr int kSignedHeaderBytes = 42;

__device__ __forceinline__ bool has_streaminfo(const unsigned char* b) {
    return b[0] == 'f' && b[1] == 'L' && b[2] == 'a' && b[3] == 'C' && (b[4] & 0x7f) == 0 && b[5] == 0 && b[6] == 0 && b[7] == 34;
}

// status: -2 not checkable (no STREAMINFO where the stream should start, another channel count than the call's, or not
// 32 bits per sample: libFLAC hashes those at ceil(bps / 8) bytes per sample), -1 unsigned (sixteen zero bytes), 0 to be
// decided by md5_compare_kernel.  counts[0] / counts[1]: streams of status 0 / of status 0 or -1.
FA_GLOBAL __global__ __launch_bounds__(256) void md5_classify_kernel(const unsigned char* __restrict__ bytes, int64_t n_bytes,
                                                                     const int64_t* __restrict__ starts, const int64_t* __restrict__ nbytes,
                                                                     int64_t n_stream, int channels, int8_t* __restrict__ status,
                                                                     int* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_stream) return;
    const int64_t at = starts[s], len = nbytes[s];
    int8_t r = -2;
    if (at >= 0 && len >= kSignedHeaderBytes && at + len <= n_bytes) {
        const unsigned char* b = bytes + at;
        if (has_streaminfo(b)) {
            const int ch = ((b[20] >> 1) & 7) + 1;
            const int bps = (((b[20] & 1) << 4) | (b[21] >> 4)) + 1;
            if (ch == channels && bps == 32) {
                unsigned any = 0;
                for (int i = 0; i < 16; ++i) any |= b[kMd5Offset + i];
                r = any ? 0 : -1;
            }
        }
    }
    status[s] = r;
    if (r == 0) atomicAdd(counts, 1);
    if (r >= -1) atomicAdd(counts + 1, 1);
}

FA_GLOBAL __global__ __launch_bounds__(256) void md5_compare_kernel(const unsigned char* __restrict__ bytes, const int64_t* __restrict__ starts,
                                                                    int64_t n_stream, unsigned char* __restrict__ digest,
                                                                    int8_t* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_stream) return;
    if (status[s] == -2)  // (decoded along with the others, but its 32-bit image is not what its signature covers)
        for (int i = 0; i < 16; ++i) digest[s * 16 + i] = 0;
    if (status[s] != 0) return;
    const unsigned char* b = bytes + starts[s] + kMd5Offset;
    unsigned diff = 0;
    for (int i = 0; i < 16; ++i) diff |= (unsigned)(b[i] ^ digest[s * 16 + i]);
    status[s] = diff ? 0 : 1;
}

FA_GLOBAL __global__ __launch_bounds__(256) void sign_check_kernel(const unsigned char* __restrict__ bytes, int64_t n_bytes,
                                                                   const int64_t* __restrict__ starts, int64_t n_stream, int* __restrict__ err) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_stream) return;
    const int64_t at = starts[s];
    if (at < 0 || at + kSignedHeaderBytes > n_bytes || !has_streaminfo(bytes + at)) atomicOr(err, 1);
}

// one thread per digest byte
FA_GLOBAL __global__ __launch_bounds__(256) void sign_streams_kernel(unsigned char* __restrict__ bytes, const int64_t* __restrict__ starts,
                                                                     int64_t n_stream, const unsigned char* __restrict__ digest) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_stream * 16) return;
    bytes[starts[i >> 4] + kMd5Offset + (i & 15)] = digest[i];
}

}  // namespace fa
