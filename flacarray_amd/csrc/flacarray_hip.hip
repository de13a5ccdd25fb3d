// flacarray_hip.hip -- host side of the C ABI declared in include/flacarray_hip.h.
//
// Plumbing semantics follow the reference's C layer: argument validation and error bits of
// encode() (src/flacarray/libflacarray/compress.c:133-156) and decode()
// (decompress.c:194-222), malloc()'d output blob owned by the caller (compress.c:251,414),
// starts = exclusive prefix sum of stream sizes (compress.c:402-429).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include <sys/mman.h>
#include <time.h>
#include <unistd.h>

#include "../../include/flacarray_hip.h"
#include "decode_kernels.hpp"
#ifndef FA_SPLIT_UNITS
#define FA_HAVE_K5_LAUNCHERS 1  // single-unit build: the K5 kernels and their launchers live here
#endif
#include "encode_kernels.hpp"
#include "encode_fused.hpp"
#include "encode_placed.hpp"
#include "decode_latency.hpp"
#include "quantize_kernels.hpp"
#include "verify_kernels.hpp"
#include "std_kernels.hpp"
#include "splice_kernels.hpp"
#include "md5_kernels.hpp"
#include "reduce_kernels.hpp"
#include "histogram_kernels.hpp"
#include "find_kernels.hpp"
#include "xsum_kernels.hpp"
#include "dot_kernels.hpp"
#include "scrub_kernels.hpp"
#include "reindex_kernels.hpp"
#include "window_kernels.hpp"
#include "join_kernels.hpp"

namespace {

using namespace fa;

#define FA_HIP_TRY(expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "flacarray_hip: %s failed: %s\n", #expr, hipGetErrorString(e_)); \
            return FA_ERROR_DEVICE;                                                               \
        }                                                                                         \
    } while (0)

// Per-device state.  Every compute entry point runs under the api_mu of the CURRENT device (the calls of one
// device share its cached scratch buffers); calls that target different devices -- one process driving several
// GPUs from several threads -- do not serialise each other.  g_mu guards the map of device states only.
constexpr int kProfPairs = 6;
constexpr int kScratchSlots = 23;
struct DeviceState {
    std::recursive_mutex api_mu;
    std::map<int, float*> windows;  // blocksize -> device tukey(0.5) table
    uint16_t* crc_tab = nullptr;
    uint16_t* crc_tab_fused = nullptr;
    // [10]: K1a partial ranges; [12]: std chunk sums and means, [13]: std summation plans (fa_stream_std_*_device);
    // [14]: the MD5 check's decoded column chunk, [15]: its chaining states, digests and flags (fa_check_md5_device);
    // [16]: the binned reduction's decoded column chunk (fa_reduce_*);
    // [17]: the damage map's realigned blob, [18]: its tolerant stream table, flags and error block, [19]: its tolerant frame
    // table, [20]: the salvage decode's task table, [21]: its fill ranges (fa_frame_status_device, fa_decode_salvage_*);
    // [22]: the reindex's error word and total (fa_reindex_device; its realigned source blob is the decoders', [7])
    void* scratch[kScratchSlots] = {};
    size_t scratch_bytes[kScratchSlots] = {};
    uint64_t scratch_epoch = 1;  // bumped whenever a scratch slot is (re)allocated or released: cached contents are then stale
    // frame-header table of the most recent encode geometry (host copy + what the device copy was built from)
    std::vector<uint4> h_hdr;
    int64_t c_nf = -1;
    int c_B = 0, c_tail = 0, c_nch = 0;
    void* c_dp = nullptr;
    uint64_t c_epoch = 0;
    bool stamps_zeroed = false;
    // (stream_size, chunk) whose summation plans scratch[13] holds, valid while scratch_epoch == std_plan_epoch
    int64_t std_plan_key[2] = {-1, -1};
    uint64_t std_plan_epoch = 0;
    int debug_fill = -1;  // fa_debug_scratch_fill: the byte every newly allocated slot is filled with, -1 = none (the default)
    hipStream_t feed_stream = nullptr;  // the host entry points' upload stream (created once: a new stream costs tens of ms)
    // small reads that want their samples on the host: the latency decoder stores them (and its status word) straight
    // into this pinned, device-visible buffer -- no copy calls, one stream synchronisation (decode_device_impl)
    void* pin = nullptr;
    void* pin_dev = nullptr;
    bool pin_tried = false;
    // the frame CRC-16 check of a large decode runs beside K7 on this stream (run_verify_beside)
    hipStream_t verify_stream = nullptr;
    hipEvent_t verify_ev[2] = {nullptr, nullptr};
    bool verify_tried = false;
    // optional in-library kernel timing (HIP events on the launch stream), see fa_profile_enable
    // pairs: 0 K3 encode_frames, 1 K5 compact_frames, 2 K7 decode_frames, 3 whole encode sequence (begin .. finish),
    // 4 whole decode sequence (K6 + K7 + checks), 5 K1 float32_to_int32
    hipEvent_t ev[2 * kProfPairs];
    bool ev_ready = false;
    bool ev_set[kProfPairs] = {false, false, false, false, false, false};
};
std::mutex g_mu;
std::map<int, std::unique_ptr<DeviceState>> g_dev;
std::atomic<bool> g_prof{false};
std::atomic<bool> g_verify{false};  // fa_set_decode_verify: re-compute every decoded frame's CRC-16
std::atomic<bool> g_encode_verify{false};  // fa_set_encode_verify: the host encoders compare each chunk's streams with its input
std::atomic<bool> g_encode_md5{false};  // fa_set_encode_md5: the host encoders sign each chunk's streams (STREAMINFO MD5)

DeviceState* dev_state() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    auto& p = g_dev[d];
    if (!p) p.reset(new DeviceState());
    return p.get();
}
#define FA_API_LOCK_OR(fail_stmt)      \
    DeviceState* ds_ = dev_state();    \
    if (!ds_) { fail_stmt; }           \
    std::lock_guard<std::recursive_mutex> api_lock_(ds_->api_mu)
#define FA_API_LOCK FA_API_LOCK_OR(return FA_ERROR_DEVICE)

// the reference's restore functions return void (flacarray.h:295-311): a device failure cannot be reported to the
// caller, and returning garbage silently is worse than stopping -- say which call failed, then abort
[[noreturn]] void fatal_device(const char* fn, const char* what) {
    std::fprintf(stderr, "flacarray_hip: %s: %s failed (%s); this entry point has no error channel and no CPU fallback\n", fn, what,
                 hipGetErrorString(hipGetLastError()));
    std::abort();
}

void prof_begin(int k, hipStream_t st) {
    if (!g_prof) return;
    DeviceState* ds = dev_state();
    if (!ds) return;
    if (!ds->ev_ready) {
        for (auto& e : ds->ev) (void)hipEventCreate(&e);
        ds->ev_ready = true;
    }
    (void)hipEventRecord(ds->ev[2 * k], st);
}
void prof_end(int k, hipStream_t st) {
    if (!g_prof) return;
    DeviceState* ds = dev_state();
    if (!ds) return;
    (void)hipEventRecord(ds->ev[2 * k + 1], st);
    ds->ev_set[k] = true;
}

// grow-only cached device scratch of the current device; slot selects independent buffers (callers hold api_mu)
int get_scratch(int slot, size_t bytes, void** out) {
    DeviceState* st = dev_state();
    if (!st) return FA_ERROR_DEVICE;
    if (st->scratch_bytes[slot] < bytes) {
        if (st->scratch[slot]) (void)hipFree(st->scratch[slot]);
        st->scratch[slot] = nullptr;
        st->scratch_bytes[slot] = 0;
        st->scratch_epoch++;
        size_t want = bytes + (bytes >> 3) + 256;
        if (hipMalloc(&st->scratch[slot], want) != hipSuccess) {
            if (hipMalloc(&st->scratch[slot], bytes) != hipSuccess) return FA_ERROR_ALLOC | FA_ERROR_DEVICE;
            want = bytes;
        }
        st->scratch_bytes[slot] = want;
        if (st->debug_fill >= 0) {  // fa_debug_scratch_fill (tests): a fresh slot starts as dirty as the held ones
            if (hipMemset(st->scratch[slot], st->debug_fill, want) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FA_ERROR_DEVICE;
        }
    }
    *out = st->scratch[slot];
    return FA_ERROR_NONE;
}

// tukey(0.5) window of length L (libFLAC's default apodization for levels 3-5)
void tukey_window(int L, std::vector<float>& w) {
    w.assign((size_t)L, 1.0f);
    const int Np = (int)(0.25f * (float)L) - 1;
    if (Np > 0) {
        for (int n = 0; n <= Np; ++n) {
            w[(size_t)n] = (float)(0.5 - 0.5 * std::cos(3.14159265358979323846 * (double)n / (double)Np));
            w[(size_t)(L - Np - 1 + n)] = (float)(0.5 - 0.5 * std::cos(3.14159265358979323846 * (double)(n + Np) / (double)Np));
        }
    }
}

int get_window(int L, const float** out) {
    DeviceState* st = dev_state();
    if (!st) return FA_ERROR_DEVICE;
    auto it = st->windows.find(L);
    if (it == st->windows.end()) {
        std::vector<float> w;
        tukey_window(L, w);
        float* d = nullptr;
        FA_HIP_TRY(hipMalloc(&d, sizeof(float) * (size_t)(L + 16)));
        FA_HIP_TRY(hipMemset(d, 0, sizeof(float) * (size_t)(L + 16)));
        FA_HIP_TRY(hipMemcpy(d, w.data(), sizeof(float) * (size_t)L, hipMemcpyHostToDevice));
        it = st->windows.emplace(L, d).first;
    }
    *out = it->second;
    return FA_ERROR_NONE;
}

// CRC-16 (poly 0x8005) tables for compact_frames_kernel, see encode_kernels.hpp
int get_crc_tab(const uint16_t** out) {
    DeviceState* st = dev_state();
    if (!st) return FA_ERROR_DEVICE;
    if (!st->crc_tab) {
        std::vector<uint16_t> t((size_t)kCrcTabWords);
        auto feed = [](uint16_t c, uint8_t v) { return crc16_byte(c, v); };
        for (int k = 0; k < 4; ++k)
            for (int v = 0; v < 256; ++v) {
                uint16_t c = 0;
                for (int b = 0; b < 4; ++b) c = feed(c, (uint8_t)(b == k ? v : 0));
                t[(size_t)(k * 256 + v)] = c;
            }
        for (int v = 0; v < 256; ++v) {
            uint16_t hi = (uint16_t)(v << 8), lo = (uint16_t)v;
            for (int b = 0; b < 256; ++b) { hi = feed(hi, 0); lo = feed(lo, 0); }
            t[(size_t)(1024 + v)] = hi;
            t[(size_t)(1280 + v)] = lo;
        }
        uint16_t xp = 1;  // x^0
        for (int n = 0; n < 512; ++n) {
            t[(size_t)(1536 + n)] = xp;
            xp = feed(xp, 0);  // multiply by x^8
        }
        uint16_t* d = nullptr;
        FA_HIP_TRY(hipMalloc(&d, sizeof(uint16_t) * (size_t)kCrcTabWords));
        FA_HIP_TRY(hipMemcpy(d, t.data(), sizeof(uint16_t) * (size_t)kCrcTabWords, hipMemcpyHostToDevice));
        st->crc_tab = d;
    }
    *out = st->crc_tab;
    return FA_ERROR_NONE;
}

// CRC-16 tables of the single-pass encoder (encode_fused.hpp): four slicing tables pre-multiplied by x^2016, so that
// XORing a lane's running state into the top half of its next word (256 bytes further on) advances it for free,
// followed by xpow[i] = x^(8 (i - 255)) mod P for the final per-lane alignment (negative powers through the order of
// x^8 in GF(2)[x] / P, found by iteration).
int get_crc_tab_fused(const uint16_t** out) {
    DeviceState* st = dev_state();
    if (!st) return FA_ERROR_DEVICE;
    if (!st->crc_tab_fused) {
        std::vector<uint16_t> t((size_t)(kFCrcSlice + kFCrcXpow));
        auto mulx8 = [](uint16_t c) { return crc16_byte(c, 0); };
        auto mulmod = [](uint16_t a, uint16_t b) {
            uint32_t r = 0;
            for (int i = 15; i >= 0; --i) {
                r = (r << 1) ^ ((r & 0x8000u) ? 0x18005u : 0u);
                if ((b >> i) & 1) r ^= a;
            }
            return (uint16_t)r;
        };
        int ord = 0;
        for (uint16_t c = 1;;) { c = mulx8(c); ++ord; if (c == 1) break; }
        auto xpow8 = [&](long k) {  // x^(8k) mod P for any integer k
            k %= ord;
            if (k < 0) k += ord;
            uint16_t c = 1;
            for (long i = 0; i < k; ++i) c = mulx8(c);
            return c;
        };
        const uint16_t x2016 = xpow8(252);
        for (int k = 0; k < 4; ++k)
            for (int v = 0; v < 256; ++v) {
                uint16_t c = 0;
                for (int b = 0; b < 4; ++b) c = crc16_byte(c, (uint8_t)(b == k ? v : 0));
                t[(size_t)(k * 256 + v)] = mulmod(c, x2016);
            }
        {
            uint16_t c = xpow8(-255);
            for (int i = 0; i < kFCrcXpow; ++i) { t[(size_t)(kFCrcSlice + i)] = c; c = mulx8(c); }
        }
        uint16_t* d = nullptr;
        FA_HIP_TRY(hipMalloc(&d, sizeof(uint16_t) * t.size()));
        FA_HIP_TRY(hipMemcpy(d, t.data(), sizeof(uint16_t) * t.size(), hipMemcpyHostToDevice));
        st->crc_tab_fused = d;
    }
    *out = st->crc_tab_fused;
    return FA_ERROR_NONE;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- the encode driver's plan: what every encode sequence, size query and splice derives from a geometry ----
// Validation in the order of the reference's encode() (compress.c:144-152), then the two limits of the format and the
// grid.  On FA_ERROR_ENCODE_PROCESS (a limit) P, B, nf and tail_bs are set; on the argument errors nothing is.
struct FramePlan {
    LevelParams P;
    uint32_t level;
    int nch;
    int64_t n_stream, stream_size;
    int64_t B, nf, F, hb;  // block size, frames per stream, frames, stream header bytes
    int tail_bs;           // samples of a stream's last frame
    int64_t slot_stride;   // one slot per frame: kSlotBytes per channel
    int64_t capacity;      // every frame VERBATIM: one slot per frame and channel + the stream headers
    int32_t pmax_full, pmax_tail;     // max_porder_for(B / tail_bs, max_porder, 0)
    double escale_full, escale_tail;  // 0.5 / blocksize
};

int make_frame_plan(int64_t n_stream, int64_t stream_size, uint32_t level, int nch, FramePlan* fp) {
    if (level > 8) return FA_ERROR_INVALID_LEVEL;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    fp->P = level_params(level);
    fp->level = level; fp->nch = nch; fp->n_stream = n_stream; fp->stream_size = stream_size;
    fp->B = fp->P.blocksize;
    fp->nf = (stream_size + fp->B - 1) / fp->B;
    fp->tail_bs = (int)(stream_size - (fp->nf - 1) * fp->B);
    if (18 * fp->nf >= (1 << 24)) return FA_ERROR_ENCODE_PROCESS;  // SEEKTABLE block length is 24 bit
    if (fp->nf > 0x7fffffffLL / n_stream) return FA_ERROR_ENCODE_PROCESS;  // 32-bit frame numbers (the grid; K3G's tickets: + its grid, still 32 bit); the host API chunks
    fp->F = n_stream * fp->nf;
    fp->hb = stream_header_bytes(fp->nf);
    fp->slot_stride = (int64_t)kSlotBytes * nch;
    fp->capacity = fp->F * fp->slot_stride + n_stream * fp->hb;
    fp->pmax_full = max_porder_for((int)fp->B, fp->P.max_porder, 0);
    fp->pmax_tail = max_porder_for(fp->tail_bs, fp->P.max_porder, 0);
    fp->escale_full = 0.5 / (double)fp->B;
    fp->escale_tail = 0.5 / (double)fp->tail_bs;
    return FA_ERROR_NONE;
}

// the slot sequence (K3 + K4 + K5): a slot per frame, the frame sizes and offsets, the stream sizes, the total
struct SlotLayout {
    size_t off_slots, off_fbytes, off_foff, off_snb, off_total, total;
};
SlotLayout slot_layout(const FramePlan& fp) {
    SlotLayout l;
    size_t o = 0;
    l.off_slots = o;  o = align_up(o + (size_t)fp.F * (size_t)fp.slot_stride, 256);
    l.off_fbytes = o; o = align_up(o + (size_t)fp.F * 4, 256);
    l.off_foff = o;   o = align_up(o + (size_t)fp.F * 8, 256);
    l.off_snb = o;    o = align_up(o + (size_t)fp.n_stream * 8, 256);
    l.off_total = o;  o = align_up(o + 8, 256);
    l.total = o + 4096;  // slack: the compaction kernel reads whole groups of 256-byte blocks past a frame's end
    return l;
}

template <int MLO, int NCH>
void launch_encode(const EncodeArgs& a, int64_t F, hipStream_t st) {
    hipLaunchKernelGGL((encode_frames_kernel<MLO, NCH>), dim3((unsigned)F), dim3(64), 0, st, a);
}
// K3 by the level's maximal LPC order and the channel count, `grid` workgroups
void launch_encode_for(const EncodeArgs& a, int nch, int64_t grid, hipStream_t st) {
#ifdef FA_DEV_MINIMAL  // diagnostic builds (seconds instead of minutes to compile): level 3-5 int32 kernels only
    (void)nch;
    launch_encode<8, 1>(a, grid, st);
#else
    if (nch == 1) {
        switch (a.max_lpc_order) {
            case 0: launch_encode<0, 1>(a, grid, st); break;
            case 6: launch_encode<6, 1>(a, grid, st); break;
            case 8: launch_encode<8, 1>(a, grid, st); break;
            default: launch_encode<12, 1>(a, grid, st); break;
        }
    } else {
        switch (a.max_lpc_order) {
            case 0: launch_encode<0, 2>(a, grid, st); break;
            case 6: launch_encode<6, 2>(a, grid, st); break;
            case 8: launch_encode<8, 2>(a, grid, st); break;
            default: launch_encode<12, 2>(a, grid, st); break;
        }
    }
#endif
}

// The publish block of the single-pass encoders' workspace (K3F and K3G): frame sizes and absolute offsets, then the
// words the kernels publish through -- sizes, offsets, and 256 bytes that hold the ticket word (+0), the error flags
// (+8), K3F's NaN flag (+12) and the scanner's total (+16: next to the error word, one copy brings all three back).
struct PublishBlock {
    size_t off_fbytes, off_fabs, off_zero, off_size, off_off, off_ticket, zero_bytes, off_total;
};
// lays the block out from offset 0 and returns its end
size_t lay_publish_block(int64_t F, PublishBlock* b) {
    size_t o = 0;
    b->off_fbytes = o; o = align_up(o + (size_t)F * 4, 256);
    b->off_fabs = o;   o = align_up(o + (size_t)F * 8, 256);
    b->off_zero = o;   // everything from here to off_total is zeroed before every launch
    b->off_size = o;   o = align_up(o + (size_t)F * 4, 256);
    b->off_off = o;    o = align_up(o + (size_t)F * 8, 256);
    b->off_ticket = o; o = align_up(o + 32, 256);
    b->zero_bytes = o - b->off_zero;
    b->off_total = o;  o = align_up(o + 8, 256);
    return o;
}
void point_into_publish_block(const PublishBlock& b, char* ws, FusedArgs* a) {
    a->frame_bytes = reinterpret_cast<uint32_t*>(ws + b.off_fbytes);
    a->frame_abs = reinterpret_cast<int64_t*>(ws + b.off_fabs);
    a->size_pub = reinterpret_cast<uint32_t*>(ws + b.off_size);
    a->off_pub = reinterpret_cast<unsigned long long*>(ws + b.off_off);
    a->ticket = reinterpret_cast<uint32_t*>(ws + b.off_ticket);
    a->err = reinterpret_cast<int*>(ws + b.off_ticket + 8);
    a->total = reinterpret_cast<int64_t*>(ws + b.off_ticket + 16);
}

// ---- single-pass encode (encode_fused.hpp): every frame is a full 4096-sample mono frame ----
struct FusedLayout {
    PublishBlock pub;
    size_t off_tslots, off_tbytes, off_toff, off_tzero;  // short last frames: slots and the compaction's arguments
    size_t total;
};

static bool slots_forced() { return std::getenv("FLACARRAY_HIP_SLOTS") != nullptr; }  // diagnostic: K3 + K4 + K5 for everything
// f32: float32 input (quantised in the staging load of K3F only: whole frames).  int32 streams may end in a short
// frame -- the slot encoder writes those, K3F the rest -- if every frame still starts on a 16-byte boundary.
bool fused_geometry(const FramePlan& fp, bool f32 = false) {
    if (fp.level < 3 || fp.nch != 1) return false;
    if (fp.tail_bs != kMaxBlock && (f32 || fp.stream_size % 4 != 0 || fp.stream_size < 2 * kMaxBlock)) return false;
    return !slots_forced();
}

FusedLayout fused_layout(const FramePlan& fp) {
    FusedLayout l;
    size_t o = lay_publish_block(fp.F, &l.pub);
    l.off_tslots = l.off_tbytes = l.off_toff = l.off_tzero = o;
    if (fp.tail_bs != kMaxBlock) {
        l.off_tslots = o; o = align_up(o + (size_t)fp.n_stream * (size_t)kSlotBytes + 4096, 256);  // (+ the compaction's group reads)
        l.off_tbytes = o; o = align_up(o + (size_t)fp.n_stream * 4, 256);
        l.off_toff = o;   o = align_up(o + (size_t)fp.n_stream * 8, 256);
        l.off_tzero = o;  o = align_up(o + (size_t)fp.n_stream * 8, 256);
    }
    l.total = o;
    return l;
}


// ---- single-pass encode of every other geometry (encode_placed.hpp): K3's frame body, frames placed by their waves ----
struct PlacedLayout {
    PublishBlock pub;
    size_t off_slots, total;
};

// the persistent grid (+ the scanner's workgroup), never more than frames + scanner
constexpr int64_t kPlacedBelowFrames = 4096;  // (see placed_preferred)
int64_t placed_grid(int64_t F) {
    int64_t g = kPlacedGrid;
    if (const char* e = std::getenv("FLACARRAY_HIP_PLACED_GRID")) {  // diagnostic: another grid (64 .. 16384 workgroups)
        const long v = std::atol(e);
        if (v >= 64 && v <= 16384) g = v;
    }
    return std::min<int64_t>(g, F) + 1;
}

PlacedLayout placed_layout(const FramePlan& fp) {
    PlacedLayout l;
    // (slots sized for the 1152-sample blocks of levels 0-2 -- 5 / 9.5 KB, L2 resident -- change nothing: 11.89 against 11.90 ms)
    size_t o = lay_publish_block(fp.F, &l.pub);
    // two slots per workgroup of the persistent grid + the placement copy's reads past the last slot's end
    l.off_slots = o;  o = align_up(o + (size_t)placed_grid(fp.F) * 2 * (size_t)fp.slot_stride + 256 * (size_t)(FA_PG_GROUP) + 256, 256);
    l.total = o;
    return l;
}

// optional CRC-16 check of every frame the decode just read (verify_kernels.hpp); h_err receives the refreshed flags
// verify: 1 = check, 0 = do not, negative = the process default (fa_set_decode_verify)
int run_verify(const DecodeArgs& a, int* d_err, int* h_err, hipStream_t st, int verify) {
    if (!(verify < 0 ? g_verify.load() : verify != 0)) return FA_ERROR_NONE;
    const uint16_t* tab = nullptr;
    int rc = get_crc_tab_fused(&tab);
    if (rc) return rc;
    hipLaunchKernelGGL(verify_crc16_kernel, dim3((unsigned)((a.n_tasks + 3) / 4)), dim3(256), 0, st, a, tab);
    FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    return FA_ERROR_NONE;
}

// The same check, issued BESIDE K7 instead of after it: K9 reads only the compressed bytes and the frame table, K7 is
// bound by the latency of its Rice chain at two waves per SIMD and leaves half of the HBM bandwidth and a third of the
// issue slots idle, and K9's waves (few registers) fit beside K7's.  begin: the side stream waits for everything queued
// on `st` so far (K6's tables), then K9 is launched on it; end: `st` waits for K9.  Both kernels report through atomics
// on the same status word.  The side stream has the lowest priority and K9 is queued AFTER K7 (queued first, its 262 144
// small workgroups take every CU and K7 starts when they are done: 7.2 + 2.9 ms, measured).  begin returns false when the
// side stream cannot be had: the caller then checks after K7 as before.
bool run_verify_beside_begin(hipStream_t st) {
    DeviceState* ds = dev_state();
    if (!ds) return false;
    if (!ds->verify_tried) {
        ds->verify_tried = true;
        hipStream_t vs = nullptr;
        int least = 0, greatest = 0;  // (numerically: least priority = the larger number)
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const char* pe = std::getenv("FLACARRAY_HIP_VERIFY_PRIO");  // experiment: "high" / "normal" instead of the lowest priority
        int prio = least;
        if (pe && pe[0] == 'h') prio = greatest;
        else if (pe && pe[0] == 'n') prio = (least + greatest) / 2;
        if (hipStreamCreateWithPriority(&vs, hipStreamNonBlocking, prio) == hipSuccess) {
            if (hipEventCreateWithFlags(&ds->verify_ev[0], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&ds->verify_ev[1], hipEventDisableTiming) == hipSuccess) {
                ds->verify_stream = vs;
            } else {
                (void)hipStreamDestroy(vs);
            }
        }
        if (!ds->verify_stream) (void)hipGetLastError();
    }
    if (!ds->verify_stream) return false;
    if (hipEventRecord(ds->verify_ev[0], st) != hipSuccess) return false;
    return hipStreamWaitEvent(ds->verify_stream, ds->verify_ev[0], 0) == hipSuccess;
}
// (called after K7 has been queued on `st`: K7's workgroups take the chip first, K9's fill what they leave)
// Returns whether K9 was queued: false means that nothing has been checked, and the caller checks after K7 as before.
bool run_verify_beside_launch(const DecodeArgs& a, hipStream_t st) {
    DeviceState* ds = dev_state();
    const uint16_t* tab = nullptr;
    if (!ds || !ds->verify_stream || get_crc_tab_fused(&tab)) return false;
    hipLaunchKernelGGL(verify_crc16_kernel, dim3((unsigned)((a.n_tasks + 3) / 4)), dim3(256), 0, ds->verify_stream, a, tab);
    (void)hipEventRecord(ds->verify_ev[1], ds->verify_stream);
    (void)hipStreamWaitEvent(st, ds->verify_ev[1], 0);
    return true;
}

constexpr size_t kPinBytes = 512u << 10;  // samples (larger results go by DMA: 1.6 MB took 307 us this way, 298 by copy); 64 bytes of status words follow
bool pinned_landing(void** host, void** dev) {
    DeviceState* ds = dev_state();
    if (!ds) return false;
    if (!ds->pin_tried) {
        ds->pin_tried = true;
        void* h = nullptr;
        void* d = nullptr;
        if (hipHostMalloc(&h, kPinBytes + 64, hipHostMallocDefault) == hipSuccess) {
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) { ds->pin = h; ds->pin_dev = d; }
            else (void)hipHostFree(h);
        } else {
            (void)hipGetLastError();
        }
    }
    *host = ds->pin;
    *dev = ds->pin_dev;
    return ds->pin != nullptr;
}

// K7L (one wavefront per frame) is used for launches of at most 4096 frames; above it the throughput decoder's 64 frames
// per wave win (K7L holds ~34 KB of LDS per frame: ~1000 frames in flight).  Measured on the benchmark data (one Rice
// partition per frame, 45-95 us each; tools/lat_crossover.py): 4000 slices = ~6000 frames 0.79 ms against K7's 1.18,
// 8000 slices 1.45 against 0.93 -- a crossover near 8000 frames; frames of 32 partitions cost K7L 0.35-0.5 ms each
// (tools/lat_sweep.py) and cross over near 2000.  4096 limits what either kind of data can lose to ~0.5 ms.
// FLACARRAY_HIP_LATENCY=0 disables it, =1 forces it for every launch of up to 65535 frames (tests).
bool latency_allowed(int64_t n_tasks) {
    const char* e = std::getenv("FLACARRAY_HIP_LATENCY");  // (read per call: the tests switch it)
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return n_tasks <= 65535;
    return n_tasks <= 4096;
}

// A decode index: what K6 derives from a store (stream metadata, the byte offset of every frame), kept in device memory
// of its own so that many reads of one store -- the reference's usage pattern, array.py:409-449 -- do not re-parse
// 4096 stream headers and rebuild a million-entry frame table per call (fa_decode_index_create).
struct DecodeIndex {
    const unsigned char* bytes = nullptr;  // the store (owned by the caller, must outlive the index)
    int64_t n_bytes = 0, n_stream = 0, stream_size = 0, nf = 0;
    int32_t B = 0, nch = 1;
    StreamMeta* meta = nullptr;
    int64_t* ftab = nullptr;
    int* err = nullptr;       // 64 ints
    void* tasks = nullptr;    // task table of the scattered-slice calls (grown on demand)
    size_t tasks_bytes = 0;
    int device = -1;
};

// A folding sink of K7 (one channel: fa_reduce_*, fa_histogram_*, fa_find_*, fa_xsum_*): what the decoded samples of the
// range are folded into where an output would stand.  The rows of the result are all streams (sel == nullptr) or the n_sel
// streams a device array names; the caller's arrays hold the identities, except the find count's and the cross-stream
// sums', which the drivers zero.  kXsum: sel is the selection sorted by group (always given) and the rows are its groups.
// kDot: sel is the selection (always given), one result row per entry, and the plan is the trivial one.
struct ReduceBins { int64_t width; ReduceOut out; };
struct FoldSink {
    enum Kind { kReduce, kHist, kFindCount, kFindFill, kXsum, kDot } kind;
    int64_t n_sel;
    const int64_t* sel;
    union {
        ReduceBins red;  // kReduce: red.out.nbins bins of `width` samples per row
        HistOut hist;    // kHist (K7H): hist.nbins value bins per row
        FindSink find;   // kFindCount, kFindFill (K7F): frame_counts, or hit_ids / offs / pos / val
        XsumSink xsum;   // kXsum (K7X): the plan's row table and sum / sq_hi / sq_lo [n_groups][n]
        DotSink dot;     // kDot (K7D): the trivial plan's row table, the template image and hi / lo [n_sel][K]
    };
};

// One decode: the store, the selection, one destination.  Each caller sets the fields it uses.
struct DecodeRequest {
    // the store: its three arrays and sizes, or an index of it (the arrays are then not looked at)
    const unsigned char* bytes = nullptr;
    const int64_t *starts = nullptr, *nbytes = nullptr;
    int64_t n_bytes = 0, n_stream = 0, stream_size = 0;
    DecodeIndex* idx = nullptr;
    int nch = 1;
    // the selection: [first, first + n_decode) of every stream (grid mode), or n_slices >= 0 slices in four host arrays
    int64_t first = 0, n_decode = 0, n_slices = -1;
    const int64_t *slice_stream = nullptr, *slice_first = nullptr, *slice_count = nullptr, *out_offset = nullptr;
    hipStream_t st = nullptr;
    int verify = -1;
    // the destination.  Device output: int32 / float32 arrays with nch == 1, int64 / float64 arrays with nch == 2 ...
    void *out_int = nullptr, *out_float = nullptr;
    const void *offsets = nullptr, *gains = nullptr;
    // ... and, with it, a host landing for a small one-channel read (*copied: the samples are at h_copy already)
    void* h_copy = nullptr;
    size_t h_copy_bytes = 0;
    bool* copied = nullptr;
    // the compare sink (first_mismatch != null): whole streams through K7 in grid mode, the caller's samples at cmp in
    // place of an output (floating point when offsets / gains are given); a frame that is rejected or cannot be located
    // marks its stream instead of setting the error word, so only errors of the stream headers are returned
    const void* cmp = nullptr;
    int64_t* first_mismatch = nullptr;
    // a folding sink (one channel): the range in grid mode over all streams, or in list mode over the streams named --
    // the sink's arrays stand where the output would be, and errors are the plain decode's
    const FoldSink* fold = nullptr;

    DecodeRequest& store(const unsigned char* b, int64_t nb, const int64_t* s, const int64_t* n, int64_t ns, int64_t size) {
        bytes = b; n_bytes = nb; starts = s; nbytes = n; n_stream = ns; stream_size = size; return *this;
    }
    DecodeRequest& slices(int64_t n, const int64_t* s, const int64_t* f, const int64_t* c, const int64_t* o) {
        n_slices = n; slice_stream = s; slice_first = f; slice_count = c; out_offset = o; return *this;
    }
    DecodeRequest& output(void* oi, void* of, const void* off, const void* g) { out_int = oi; out_float = of; offsets = off; gains = g; return *this; }
};

// what the fa_decode_* calls ask of their output arguments: exactly one array, a floating-point one with offsets and gains
int check_output_args(const void* out_int, const void* out_float, const void* offsets, const void* gains) {
    if ((out_int == nullptr) == (out_float == nullptr)) return FA_ERROR_CONVERT_TYPE;
    if (out_float && (!offsets || !gains)) return FA_ERROR_CONVERT_TYPE;
    return FA_ERROR_NONE;
}

// an index is used on the device that holds it (its tables, the store and the call's lock are that device's)
int index_on_device(const DecodeIndex* ix) {
    int cur = -1;
    return (hipGetDevice(&cur) != hipSuccess || cur != ix->device) ? FA_ERROR_DEVICE : FA_ERROR_NONE;
}

// device memory for a task table: the index's own (grown on demand) or the cached scratch
int task_table_mem(DecodeIndex* idx, size_t bytes, void** out) {
    if (!idx) return get_scratch(3, bytes, out);
    if (idx->tasks_bytes < bytes) {
        if (idx->tasks) (void)hipFree(idx->tasks);
        idx->tasks = nullptr; idx->tasks_bytes = 0;
        FA_HIP_TRY(hipMalloc(&idx->tasks, bytes + 4096));
        idx->tasks_bytes = bytes + 4096;
    }
    *out = idx->tasks;
    return FA_ERROR_NONE;
}

// K7's task table in memory: five columns [stream | frame | first | last | out offset] of n_tasks entries each, every
// column 256-byte aligned.  task_table_place: memory for a.n_tasks tasks (task_table_mem), the columns, `a` pointed at them.
size_t task_table_bytes(int64_t n_tasks) { return 5 * align_up((size_t)n_tasks * 8, 256); }
int task_table_place(DecodeIndex* idx, DecodeArgs& a, int64_t* col[5]) {
    const size_t bytes = task_table_bytes(a.n_tasks);
    void* p = nullptr;
    int rc = task_table_mem(idx, bytes, &p);
    if (rc) return rc;
    for (int k = 0; k < 5; ++k) col[k] = reinterpret_cast<int64_t*>(static_cast<char*>(p) + k * (bytes / 5));
    a.task_stream = col[0]; a.task_frame = col[1]; a.task_first = col[2]; a.task_last = col[3]; a.task_out_off = col[4];
    return FA_ERROR_NONE;
}

// a task table that so far rides in K7L's kernel arguments only: its host image, and where it goes when K7 or the CRC-16
// check, which read the table from memory, are needed after all
struct HeldTasks {
    std::vector<int64_t> host;
    void* dev = nullptr;
    bool uploaded = false;
    int upload(hipStream_t st) {
        FA_HIP_TRY(hipMemcpyAsync(dev, host.data(), host.size() * 8, hipMemcpyHostToDevice, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        uploaded = true;
        return FA_ERROR_NONE;
    }
};

// the find count's zero-fill (issued behind every refusal of the arguments: a refused count call has written nothing)
int find_zero_counts(const FindSink& fs, int64_t cells, hipStream_t st) {
    hipLaunchKernelGGL(find_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, fs.frame_counts, cells);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

// K6 as one step: the stream metadata and the byte offset of every frame of a store, into *t.
// own == false: the tables live in the cached scratch (slots 1 and 2) and are the running call's; errors the walk finds
// arrive with K7's status words.  own == true: they are hipMalloc'ed (the caller frees t->meta and t->ftab, also after an
// error) and the error word is read back here.  A store that is not 16-byte aligned is copied to slot 7 first (the
// kernels issue 16-byte loads relative to the blob base): t->bytes is what the tables refer to.
int build_decode_tables(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                        int64_t stream_size, int nch, hipStream_t st, bool own, DecodeIndex* t) {
    int rc = FA_ERROR_NONE;
    int h_err[4] = {0, 0, 0, 0};
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) {
        void* al = nullptr;
        if ((rc = get_scratch(7, (size_t)n_bytes + 256, &al))) return rc;
        FA_HIP_TRY(hipMemcpyAsync(al, d_bytes, (size_t)n_bytes, hipMemcpyDeviceToDevice, st));
        d_bytes = reinterpret_cast<const unsigned char*>(al);
    }
    // ---- parse stream headers ----
    prof_begin(4, st);
    void* p = nullptr;
    const size_t meta_bytes = align_up((size_t)n_stream * sizeof(StreamMeta), 256);
    if (own) {
        FA_HIP_TRY(hipMalloc(&p, meta_bytes + 256 + (size_t)n_stream * 4));
        t->meta = reinterpret_cast<StreamMeta*>(p);
    } else {
        if ((rc = get_scratch(1, meta_bytes + 256 + (size_t)n_stream * 4, &p))) return rc;
    }
    StreamMeta* d_meta = reinterpret_cast<StreamMeta*>(p);
    // [0]=err [1]=variant flags [2]=streams without a seek table [3]=scan passes of the longest of them
    int* d_err = reinterpret_cast<int*>(reinterpret_cast<char*>(p) + meta_bytes);
    int* d_sflag = d_err + 64;  // per stream: 1 = sync scan ambiguous, walk serially
    FA_HIP_TRY(hipMemsetAsync(d_err, 0, 32, st));  // ([4]: the latency kernel's "repeat with K7" flag)
    hipLaunchKernelGGL(parse_streams_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, d_bytes, d_starts,
                       d_nbytes, n_stream, stream_size, n_bytes, d_meta, d_err);
    StreamMeta m0;
    FA_HIP_TRY(hipMemcpyAsync(&m0, d_meta, sizeof(StreamMeta), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    if (h_err[0]) return h_err[0];
    const int32_t B = m0.B;
    if (m0.channels != nch) return FA_ERROR_DECODE_INIT;  // an int32 stream read as int64 or the reverse
    if (B <= 0 || B > 65535) return FA_ERROR_DECODE_INIT;
    if (B > kMaxBlock * 16) return FA_ERROR_DECODE_INIT;
    const int64_t nf = (stream_size + B - 1) / B;

    // ---- frame table ----
    void* pt = nullptr;
    if (own) {
        FA_HIP_TRY(hipMalloc(&pt, (size_t)n_stream * (size_t)nf * 8 + 256));
        t->ftab = reinterpret_cast<int64_t*>(pt);
    } else {
        if ((rc = get_scratch(2, (size_t)n_stream * (size_t)nf * 8 + 256, &pt))) return rc;
    }
    int64_t* d_ftab = reinterpret_cast<int64_t*>(pt);
    const int64_t nt = n_stream * nf;
    hipLaunchKernelGGL(build_frame_table_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, d_bytes, d_meta, n_stream,
                       nf, B, nch, d_ftab, d_err);
    if (h_err[2] > 0) {
        const bool scan = (std::getenv("FLACARRAY_HIP_NO_SYNC_SCAN") == nullptr);  // diagnostic: force the serial walk
        if (scan) {
            FA_HIP_TRY(hipMemsetAsync(d_sflag, 0, (size_t)n_stream * 4, st));
            const unsigned ny = (unsigned)(h_err[3] < 1 ? 1 : (h_err[3] > 65535 ? 65535 : h_err[3]));
            hipLaunchKernelGGL(scan_sync_kernel, dim3((unsigned)n_stream, ny), dim3(256), 0, st, d_bytes, n_bytes, d_meta, nf, B,
                               stream_size, d_ftab, d_sflag);
            hipLaunchKernelGGL(check_scan_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, d_meta, n_stream, nf, B,
                               d_ftab, d_sflag);
        }
        hipLaunchKernelGGL(walk_frames_kernel, dim3((unsigned)((n_stream + 63) / 64)), dim3(64), 0, st, d_bytes, n_bytes, d_meta,
                           n_stream, nf, B, stream_size, d_ftab, scan ? d_sflag : (const int*)nullptr, d_err);
    }
    if (own) {
        FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        FA_HIP_TRY(hipGetLastError());
        if (h_err[0]) return h_err[0];
    }
    t->bytes = d_bytes; t->n_bytes = n_bytes; t->n_stream = n_stream; t->stream_size = stream_size; t->nf = nf;
    t->B = B; t->nch = nch; t->meta = d_meta; t->ftab = d_ftab; t->err = d_err;
    return FA_ERROR_NONE;
}

// K7's launch, written once: the sink picks the specialisation of the <MO, MO_DONE> history pass.  f32: floating-point
// output (or, compare sink, floating-point samples to compare with).
template <int MO, int MO_DONE>
void launch_k7(const DecodeArgs& a, int nch, bool cmp, bool f32, const FoldSink* fold, hipStream_t st) {
    const dim3 grid((unsigned)((a.n_tasks + 63) / 64)), block(64);
#define FA_K7(...) hipLaunchKernelGGL((decode_frames_kernel<MO, MO_DONE, __VA_ARGS__>), grid, block, 0, st, a, a.err + 1)
#ifdef FA_DEV_MINIMAL
    (void)nch; (void)cmp; (void)f32; (void)fold;
    FA_K7(false, 1);
#else
    // (two channels, compare: the same decode, but a frame it rejects marks its stream -- K8C cannot tell a frame abandoned half way)
    if (nch == 2) { if (cmp) FA_K7(false, 2, true); else FA_K7(false, 2); }
    else if (fold && fold->kind == FoldSink::kFindFill) FA_K7(false, 1, false, false, false, 2);
    else if (fold && fold->kind == FoldSink::kFindCount) FA_K7(false, 1, false, false, false, 1);
    else if (fold && fold->kind == FoldSink::kHist) FA_K7(false, 1, false, false, true);
    else if (fold && fold->kind == FoldSink::kXsum) FA_K7(false, 1, false, false, false, 0, true);
    else if (fold && fold->kind == FoldSink::kDot) FA_K7(false, 1, false, false, false, 0, false, kDotKT);
    else if (fold) FA_K7(false, 1, false, true);
    else if (cmp) { if (f32) FA_K7(true, 1, true); else FA_K7(false, 1, true); }
    else if (f32) FA_K7(true, 1);
    else FA_K7(false, 1);
#endif
#undef FA_K7
}

// K7L: one wavefront per frame (decode_latency.hpp).  A launch with fewer frames than the chip has lanes is latency bound
// in K7 (one lane per frame: ~1 ms whatever the count).  Returns the call's result, or, with *repeat set, nothing yet:
// a frame K7L does not take has set the flag and the whole launch is repeated by K7.
int decode_latency_route(const DecodeRequest& r, const DecodeArgs& a, const LatInline& inl, HeldTasks& held, bool& err_cleared, bool* repeat) {
    *repeat = false;
    hipStream_t st = r.st;
    int* d_err = a.err;
    const int nch = r.nch;
    const bool flt = (r.out_float != nullptr);
    int rc = FA_ERROR_NONE;
    LatWide wd;
    std::memset(&wd, 0, sizeof wd);
    if (nch == 2) {
        wd.out_i64 = static_cast<int64_t*>(r.out_int); wd.out_f64 = static_cast<double*>(r.out_float);
        wd.offsets = static_cast<const double*>(r.offsets); wd.gains = static_cast<const double*>(r.gains);
    }
    auto launch_latency = [&](const DecodeArgs& aa, int* flag) {
        const dim3 grid((unsigned)a.n_tasks), block(64);
        if (nch == 2) {
            if (flt) hipLaunchKernelGGL((decode_latency_kernel<true, 2>), grid, block, 0, st, aa, inl, wd, flag);
            else hipLaunchKernelGGL((decode_latency_kernel<false, 2>), grid, block, 0, st, aa, inl, wd, flag);
        } else {
            if (flt) hipLaunchKernelGGL((decode_latency_kernel<true, 1>), grid, block, 0, st, aa, inl, wd, flag);
            else hipLaunchKernelGGL((decode_latency_kernel<false, 1>), grid, block, 0, st, aa, inl, wd, flag);
        }
    };
    const bool verifying = (r.verify < 0 ? g_verify.load() : r.verify != 0);
    void *pin_h = nullptr, *pin_d = nullptr;
    void* const h_copy = r.h_copy;
    const size_t h_copy_bytes = r.h_copy_bytes;
    // (the caller's own buffer, if it is pinned and device-visible -- fa_pinned_alloc, any hipHostMalloc --, takes
    // the samples directly whatever their size; otherwise the library's landing buffer, for results up to 512 KB)
    void* direct = nullptr;
    if (nch == 1 && h_copy && h_copy_bytes && !verifying) {
        hipPointerAttribute_t at;
        // (up to 2 MB: beyond that the kernel's 256-byte stores over the link are slower than one DMA copy out of
        // the device buffer; at 16 MB the two cost the same, 1.04 ms per 1000-slice read, a quarter of it the Python list of results)
        if (hipPointerGetAttributes(&at, h_copy) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
            if (h_copy_bytes <= (2u << 20)) direct = at.devicePointer;
        } else {
            (void)hipGetLastError();
        }
    }
    if (nch == 1 && h_copy && h_copy_bytes && (direct || h_copy_bytes <= kPinBytes) && !verifying && pinned_landing(&pin_h, &pin_d)) {
        // a small read that wants its samples on the host: the kernel stores them and its status word into pinned
        // host memory; what is left for the host is one synchronisation and a memcpy of a few KB
        DecodeArgs ap = a;
        void* const land = direct ? direct : pin_d;
        if (flt) ap.out_f32 = reinterpret_cast<float*>(land); else ap.out_i32 = reinterpret_cast<int32_t*>(land);
        volatile int* status = reinterpret_cast<volatile int*>(reinterpret_cast<char*>(pin_h) + kPinBytes);
        status[0] = 0;
        int* d_status = reinterpret_cast<int*>(reinterpret_cast<char*>(pin_d) + kPinBytes);
        prof_begin(2, st);
        launch_latency(ap, d_status);
        prof_end(2, st);
        prof_end(4, st);
        FA_HIP_TRY(hipStreamSynchronize(st));
        FA_HIP_TRY(hipGetLastError());
        if (status[0] == 0) {
            if (!direct) std::memcpy(h_copy, pin_h, h_copy_bytes);
            if (r.copied) *r.copied = true;
            return FA_ERROR_NONE;
        }
        // (a frame the latency decoder does not take: the whole launch again, the ordinary way)
    }
    if (!err_cleared) { FA_HIP_TRY(hipMemsetAsync(d_err, 0, 32, st)); err_cleared = true; }
    prof_begin(2, st);
    launch_latency(a, d_err + 4);
    prof_end(2, st);
    prof_end(4, st);
    int h8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (h_copy && h_copy_bytes) {
        // a small read wants its samples on the host: they travel with the status words, one synchronisation for both
        FA_HIP_TRY(hipMemcpyAsync(h_copy, flt ? (const void*)a.out_f32 : (const void*)a.out_i32, h_copy_bytes, hipMemcpyDeviceToHost, st));
    }
    FA_HIP_TRY(hipMemcpyAsync(h8, d_err, 32, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (inl.n > 0 && (h8[4] != 0 || verifying) && (rc = held.upload(st))) return rc;  // K7 and the CRC-16 check read the task table from memory
    if (h8[4] != 0 && std::getenv("FLACARRAY_HIP_LATENCY_DEBUG"))
        std::fprintf(stderr, "flacarray_hip: latency decoder gave up (reasons %d) on a launch of %lld frames (first slice: stream %lld, sample %lld); repeating with K7\n",
                     h8[4], (long long)a.n_tasks, (long long)(r.n_slices > 0 ? r.slice_stream[0] : -1), (long long)(r.n_slices > 0 ? r.slice_first[0] : r.first));
    if (h8[4] != 0) { *repeat = true; return FA_ERROR_NONE; }
    int h_err[4] = {h8[0], 0, 0, 0};
    if ((rc = run_verify(a, d_err, h_err, st, r.verify))) return rc;
    if (r.copied) *r.copied = (h_copy && h_copy_bytes);
    return h_err[0];
}

// The decode driver: every device read, every sink.  K6's tables (the index's, or built here for this call), K7's
// arguments and task table, the K7L attempt, then K7's history passes.
int decode_device_impl(const DecodeRequest& r) {
    const bool cmp = (r.first_mismatch != nullptr);
    const FoldSink* const fold = r.fold;
    const int nch = r.nch;
    hipStream_t st = r.st;
#ifdef FA_DEV_MINIMAL
    if (cmp || fold) return FA_ERROR_CONVERT_TYPE;
#endif
    int verify = cmp ? 0 : r.verify;
    if (fold && (nch != 1 || cmp)) return FA_ERROR_CONVERT_TYPE;
    int rc = FA_ERROR_NONE;
    int h_err[4] = {0, 0, 0, 0};
    bool err_cleared = true;  // (K6 clears them)
    DecodeIndex one_off;
    const DecodeIndex* t = r.idx;
    if (t) {
        if (t->nch != nch) return FA_ERROR_DECODE_INIT;
        err_cleared = false;
        prof_begin(4, st);
        // (the status words are cleared where they are first needed: a small read that lands in pinned host memory
        // never looks at them, and a memset is a launch of its own)
    } else {
        if ((rc = build_decode_tables(r.bytes, r.n_bytes, r.starts, r.nbytes, r.n_stream, r.stream_size, nch, st, false, &one_off))) return rc;
        t = &one_off;
    }
    const int64_t n_stream = t->n_stream, stream_size = t->stream_size;
    const int32_t B = t->B;
    int* const d_err = t->err;

    // ---- K7's arguments ----
    DecodeArgs a;
    std::memset(&a, 0, sizeof a);
    LatInline inl;
    std::memset(&inl, 0, sizeof inl);
    HeldTasks held;
    a.blob = t->bytes; a.blob_bytes = t->n_bytes; a.meta = t->meta; a.ftab = t->ftab; a.nf = t->nf; a.B = B;
    a.stream_size = stream_size;
    a.err = d_err;
    if (nch == 1) {
        a.out_i32 = static_cast<int32_t*>(r.out_int); a.out_f32 = static_cast<float*>(r.out_float);
        a.offsets = static_cast<const float*>(r.offsets); a.gains = static_cast<const float*>(r.gains);
    }
    a.cmp = r.cmp; a.first_mismatch = reinterpret_cast<unsigned long long*>(r.first_mismatch);
    if (cmp) FA_HIP_TRY(hipMemsetAsync(r.first_mismatch, 0xFF, (size_t)n_stream * 8, st));  // -1: no difference (yet)
    if (r.n_slices < 0) {
        a.f0 = r.first / B;
        const int64_t f1 = (r.first + r.n_decode - 1) / B;
        a.nfr = f1 - a.f0 + 1;
        a.first = r.first;
        a.n_decode = r.n_decode;
        a.n_tasks = n_stream * a.nfr;
    } else {
        // scattered slices: one task per (slice, frame)
        int64_t n_tasks = 0;
        for (int64_t i = 0; i < r.n_slices; ++i) {
            const int64_t s = r.slice_stream[i], fst = r.slice_first[i], cnt = r.slice_count[i];
            if (s < 0 || s >= n_stream || fst < 0 || cnt <= 0 || fst + cnt > stream_size) return FA_ERROR_DECODE_SAMPLE_RANGE;
            n_tasks += (fst + cnt - 1) / B - fst / B + 1;
        }
        a.n_tasks = n_tasks;
        if (a.n_tasks == 0) return FA_ERROR_NONE;
        // a handful of frames K7L will take: the task table rides in the kernel arguments as well (no upload, no
        // synchronisation).  The conditions are those of the K7L route below -- a stream with larger blocks goes
        // straight to K7, which reads the table from memory.
        const bool ride = (n_tasks <= 8 && B <= kLatMaxBlock && latency_allowed(n_tasks));
        // one staging vector, one copy
        std::vector<int64_t> h(task_table_bytes(n_tasks) / 8);
        int64_t* hc[5];
        for (int k = 0; k < 5; ++k) hc[k] = h.data() + k * (h.size() / 5);
        int64_t tk = 0;
        for (int64_t i = 0; i < r.n_slices; ++i) {
            const int64_t s = r.slice_stream[i], fst = r.slice_first[i], cnt = r.slice_count[i];
            for (int64_t f = fst / B; f <= (fst + cnt - 1) / B; ++f, ++tk) {
                hc[0][tk] = s; hc[1][tk] = f; hc[2][tk] = fst; hc[3][tk] = fst + cnt; hc[4][tk] = r.out_offset[i];
                if (ride) { inl.stream[tk] = s; inl.frame[tk] = f; inl.first[tk] = fst; inl.last[tk] = fst + cnt; inl.out_off[tk] = r.out_offset[i]; }
            }
        }
        if (ride) inl.n = (int32_t)n_tasks;
        int64_t* col[5];
        if ((rc = task_table_place(r.idx, a, col))) return rc;
        if (!ride) {
            FA_HIP_TRY(hipMemcpyAsync(col[0], h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
            FA_HIP_TRY(hipStreamSynchronize(st));  // the host vector goes out of scope
        } else {
            held.host.swap(h);  // (uploaded only if K7 has to repeat the launch)
            held.dev = col[0];
        }
    }
    if (a.B > kMaxBlock * 16) return FA_ERROR_DECODE_INIT;
    if (fold) {
        if (r.n_slices >= 0) return FA_ERROR_CONVERT_TYPE;
        const int64_t rows = fold->sel ? fold->n_sel : n_stream;
        if (fold->kind == FoldSink::kFindCount || fold->kind == FoldSink::kFindFill) {
            // the caller sized its arrays with n_frames frames per row: nothing is written before that is known to hold
            const FindSink& fs = fold->find;
            if (fs.n_frames != a.nfr) return FA_ERROR_CONVERT_TYPE;
            if ((rows * a.nfr + 255) / 256 > 0x7fffffff) return FA_ERROR_ALLOC;
            a.find_lo = fs.lo; a.find_hi = fs.hi; a.find_inside = fs.inside ? 1 : 0;
            if (fold->kind == FoldSink::kFindFill) {
                a.find_out = fs.pos; a.find_val = fs.val; a.find_ids = fs.hit_ids; a.find_offs = fs.offs;
            } else {
                a.find_out = fs.frame_counts;
                a.red_nbins = a.nfr;  // (out_off = row * nfr, as the other folding sinks have row * nbins)
            }
        } else if (fold->kind == FoldSink::kXsum) {
            const XsumSink& xs = fold->xsum;
            if (!fold->sel || xs.n_rows <= 0 || xs.n_rows > 0x7fffffff / a.nfr) return FA_ERROR_DECODE_SAMPLE_RANGE;
            a.xs_sum = xs.sum; a.xs_sq_hi = xs.sq_hi; a.xs_sq_lo = xs.sq_lo;
        } else if (fold->kind == FoldSink::kDot) {
            const DotSink& ds = fold->dot;
            if (!fold->sel || ds.n_rows <= 0 || ds.n_rows > 0x7fffffff / a.nfr) return FA_ERROR_DECODE_SAMPLE_RANGE;
            a.dot_hi = ds.hi; a.dot_lo = ds.lo; a.dot_tmpl = ds.tmpl; a.dot_ld = ds.ld; a.dot_rows = fold->n_sel; a.dot_k = ds.K; a.dot_k0 = ds.k0;
        } else if (fold->kind == FoldSink::kHist) {
            const HistOut& ho = fold->hist;
            a.hist_counts = ho.counts; a.hist_below = ho.below; a.hist_above = ho.above; a.hist_lo = ho.lo; a.hist_shift = ho.shift;
            a.red_nbins = ho.nbins;
        } else {
            const ReduceOut& o = fold->red.out;
            a.red_min = o.mn; a.red_max = o.mx; a.red_sum = o.sum; a.red_sq_hi = o.sq_hi; a.red_sq_lo = o.sq_lo;
            a.red_width = fold->red.width; a.red_nbins = o.nbins;
        }
        if (fold->sel) a.n_tasks = fold->n_sel * a.nfr;  // list mode; the table is built on the device, below
        if (fold->kind == FoldSink::kFindFill) a.n_tasks = fold->find.n_hit;  // (the frames with a hit, always a list)
        if (fold->kind == FoldSink::kXsum) a.n_tasks = fold->xsum.n_rows * a.nfr * 64;  // (a wave per plan row and frame)
        if (fold->kind == FoldSink::kDot) a.n_tasks = fold->dot.n_rows * a.nfr * 64;    // (the same layout)
        if (a.n_tasks <= 0 || a.n_tasks > (int64_t)64 * 0x7fffffff) return FA_ERROR_DECODE_SAMPLE_RANGE;
        if (fold->kind == FoldSink::kFindCount && (rc = find_zero_counts(fold->find, rows * a.nfr, st))) return rc;
    }
    if (!cmp && !fold && a.B <= kLatMaxBlock && latency_allowed(a.n_tasks)) {
        bool repeat = false;
        rc = decode_latency_route(r, a, inl, held, err_cleared, &repeat);
        if (!repeat) return rc;
    }
    if (!err_cleared) { FA_HIP_TRY(hipMemsetAsync(d_err, 0, 32, st)); err_cleared = true; }
    // no K7 launch ever sees a task table that only exists in kernel arguments
    if (inl.n > 0 && !held.uploaded && (rc = held.upload(st))) return rc;
    if (fold && (fold->kind == FoldSink::kFindFill || fold->sel)) {
        const int64_t rows = fold->sel ? fold->n_sel : n_stream;
        int64_t* col[5];
        if ((rc = task_table_place(r.idx, a, col))) return rc;
        if (fold->kind == FoldSink::kFindFill)
            // the frames that hold a hit: task t = cell hit_ids[t], output base offs[cell]
            hipLaunchKernelGGL(find_tasks_kernel, dim3((unsigned)((a.n_tasks + 255) / 256)), dim3(256), 0, st, fold->find.hit_ids, a.n_tasks, rows,
                               a.nfr, a.f0, a.first, a.first + a.n_decode, fold->sel, n_stream, fold->find.offs, col[0], col[1], col[2], col[3],
                               col[4], d_err, (int)FA_ERROR_DECODE_SAMPLE_RANGE);
        else if (fold->kind == FoldSink::kXsum)
            // one frame of the 64 streams of a plan row per wave, output offset group * n
            hipLaunchKernelGGL(xsum_tasks_kernel, dim3((unsigned)((a.n_tasks + 255) / 256)), dim3(256), 0, st, fold->sel, fold->n_sel,
                               fold->xsum.rows, fold->xsum.n_rows, fold->xsum.n_groups, n_stream, a.nfr, a.f0, a.first, a.first + a.n_decode,
                               col[0], col[1], col[2], col[3], col[4], d_err, (int)FA_ERROR_DECODE_SAMPLE_RANGE);
        else if (fold->kind == FoldSink::kDot)
            // K7X's layout with one group: one frame of the 64 streams of a plan row per wave (the output offset is not used)
            hipLaunchKernelGGL(xsum_tasks_kernel, dim3((unsigned)((a.n_tasks + 255) / 256)), dim3(256), 0, st, fold->sel, fold->n_sel,
                               fold->dot.rows, fold->dot.n_rows, (int64_t)1, n_stream, a.nfr, a.f0, a.first, a.first + a.n_decode,
                               col[0], col[1], col[2], col[3], col[4], d_err, (int)FA_ERROR_DECODE_SAMPLE_RANGE);
        else
            // the named streams: task t = (row t / nfr, frame f0 + t % nfr), output slot row * nbins
            hipLaunchKernelGGL(reduce_tasks_kernel, dim3((unsigned)((a.n_tasks + 255) / 256)), dim3(256), 0, st, fold->sel, n_stream, a.n_tasks,
                               a.nfr, a.f0, a.first, a.first + a.n_decode, a.red_nbins, col[0], col[1], col[2], col[3], col[4], d_err,
                               (int)FA_ERROR_DECODE_SAMPLE_RANGE);
    }
    const bool f32 = cmp ? (r.offsets != nullptr) : (r.out_float != nullptr);  // (one channel)
#ifndef FA_DEV_MINIMAL
    if (nch == 2) {
        // two-channel arrays: task-local planar image (low words), bit 32 of every sample, task status
        a.hib_words = (a.B + 31) / 32;
        const size_t tmp_b = align_up((size_t)a.n_tasks * 2 * (size_t)a.B * 4, 256);
        const size_t hib_b = align_up((size_t)a.n_tasks * 2 * (size_t)a.hib_words * 4, 256);
        const size_t asg_b = align_up((size_t)a.n_tasks * 4, 256);
        void* p8 = nullptr;
        rc = get_scratch(8, tmp_b + hib_b + asg_b, &p8);
        if (rc) return rc;
        a.out_i32 = reinterpret_cast<int32_t*>(p8);
        a.out_f32 = nullptr;
        a.hibits = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(p8) + tmp_b);
        a.assign = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(p8) + tmp_b + hib_b);
        FA_HIP_TRY(hipMemsetAsync(a.assign, 0xFF, (size_t)a.n_tasks * 4, st));
        prof_begin(2, st);
        if (std::getenv("FLACARRAY_HIP_NO_VERBATIM_KERNEL") == nullptr) {  // (diagnostic: K7 alone decodes everything)
            hipLaunchKernelGGL(verbatim_channel0_kernel, dim3((unsigned)a.n_tasks), dim3(256), 0, st, a);
            a.verbatim_done = 1;
        }
        launch_k7<8, -1>(a, 2, cmp, false, nullptr, st);
        prof_end(2, st);
        FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        if (h_err[1] & kFlagNeed16) launch_k7<16, 8>(a, 2, cmp, false, nullptr, st);
        if (h_err[1]) {  // a frame left over by the 16-deep pass raises the flag again
            FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
            FA_HIP_TRY(hipStreamSynchronize(st));
        }
        if (h_err[1] & kFlagNeed32) launch_k7<32, 16>(a, 2, cmp, false, nullptr, st);
        const double* const off64 = static_cast<const double*>(r.offsets);
        const double* const gain64 = static_cast<const double*>(r.gains);
        if (cmp) hipLaunchKernelGGL(compare_channels_kernel, dim3((unsigned)a.n_tasks), dim3(256), 0, st, a, off64, gain64);
        else hipLaunchKernelGGL(combine_channels_kernel, dim3((unsigned)a.n_tasks), dim3(256), 0, st, a, static_cast<int64_t*>(r.out_int),
                                static_cast<double*>(r.out_float), off64, gain64);
        FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        FA_HIP_TRY(hipGetLastError());
        if (cmp) return h_err[0] & ~(kErrDecodeProcess | kErrDecodeSeek);
        if ((rc = run_verify(a, d_err, h_err, st, verify))) return rc;
        return h_err[0];
    }
#endif
    prof_begin(2, st);
#ifdef FA_DEV_MINIMAL
    launch_k7<8, -1>(a, 1, cmp, f32, fold, st);
    prof_end(2, st);
    prof_end(4, st);
    FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    if ((rc = run_verify(a, d_err, h_err, st, verify))) return rc;
    return h_err[0] | (h_err[1] ? FA_ERROR_DECODE_PROCESS : 0);
#else
    // the frame CRC-16 check of a launch that fills the chip goes beside K7 (it needs what K6 built, nothing of K7's)
    const bool verifying_k7 = (verify < 0 ? g_verify.load() : verify != 0);
    const bool beside = verifying_k7 && a.n_tasks >= 16384 && std::getenv("FLACARRAY_HIP_VERIFY_AFTER") == nullptr &&
                        run_verify_beside_begin(st);
    launch_k7<8, -1>(a, 1, cmp, f32, fold, st);
    prof_end(2, st);
    // (queued: the check at the end of this function is not repeated; not queued: it runs there, after K7)
    if (beside && run_verify_beside_launch(a, st)) verify = 0;
    prof_end(4, st);  // (deeper-history passes, when a stream needs them, follow outside this pair)
    FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    if (h_err[1] & kFlagNeed16) launch_k7<16, 8>(a, 1, cmp, f32, fold, st);
    if (h_err[1] & kFlagNeed32) launch_k7<32, 16>(a, 1, cmp, f32, fold, st);
    if (h_err[1]) {
        FA_HIP_TRY(hipMemcpyAsync(h_err, d_err, 16, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
    }
    FA_HIP_TRY(hipGetLastError());
    if (cmp) return h_err[0] & ~(kErrDecodeProcess | kErrDecodeSeek);
    if ((rc = run_verify(a, d_err, h_err, st, verify))) return rc;
    return h_err[0];
#endif
}

int validate_range(int64_t stream_size, int64_t first_sample, int64_t last_sample, int64_t* first_decode, int64_t* n_decode) {
    *first_decode = 0;
    *n_decode = stream_size;
    if (first_sample >= 0 && last_sample >= 0) {  // decompress.c:209-222
        if (last_sample > stream_size) return FA_ERROR_DECODE_SAMPLE_RANGE;
        if (first_sample > stream_size - 1) return FA_ERROR_DECODE_SAMPLE_RANGE;
        if (first_sample >= last_sample) return FA_ERROR_DECODE_SAMPLE_RANGE;
        *first_decode = first_sample;
        *n_decode = last_sample - first_sample;
    }
    return FA_ERROR_NONE;
}


// numpy's pairwise-sum tree of one chunk of `length` elements (flacarray_amd/npsum.py pairwise_plan): leaves (offset,
// length) in element order and the postfix combine program (1 = push the next leaf's sum, 0 = add the top two)
void std_build_plan(int64_t length, std::vector<int32_t>& leaves, std::vector<uint8_t>& ops) {
    struct Node { int64_t off, n; bool done; };
    std::vector<Node> stack{{0, length, false}};
    while (!stack.empty()) {
        const Node nd = stack.back();
        stack.pop_back();
        if (nd.n <= kStdLeaf) {
            leaves.push_back((int32_t)nd.off);
            leaves.push_back((int32_t)nd.n);
            ops.push_back(1);
        } else if (nd.done) {
            ops.push_back(0);
        } else {
            int64_t n2 = nd.n / 2;
            n2 -= n2 % 8;
            stack.push_back({nd.off, nd.n, true});
            stack.push_back({nd.off + n2, nd.n - n2, false});
            stack.push_back({nd.off, n2, false});
        }
    }
}

// fa_stream_std_f32_device / _f64_device: S1 + S2 for the sum (-> means), S1 + S2 for the squared deviations (-> std)
template <typename T>
int stream_std_impl(const T* d_in, int64_t n_stream, int64_t stream_size, int64_t chunk, T* d_out, void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    if (chunk <= 0 || chunk > INT32_MAX || stream_size > INT64_MAX / 2) return FA_ERROR_CONVERT_TYPE;
    const int64_t cps = (stream_size + chunk - 1) / chunk;
    if (n_stream > INT32_MAX / cps) return FA_ERROR_CONVERT_TYPE;  // one workgroup per chunk: the grid's bound
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t tail = stream_size - (cps - 1) * chunk;
    // plans of the chunk lengths the lane-per-leaf path does not cover
    std::vector<int32_t> lv[2];
    std::vector<uint8_t> op[2];
    if (chunk != kStdFastChunk && stream_size >= chunk) std_build_plan(chunk, lv[0], op[0]);
    if (tail != chunk && tail != kStdFastChunk) std_build_plan(tail, lv[1], op[1]);
    const size_t lv_b = 4 * (lv[0].size() + lv[1].size());
    const size_t plan_b = lv_b + op[0].size() + op[1].size();
    const size_t sums_b = ((size_t)(n_stream * cps) * sizeof(T) + 255) & ~(size_t)255;
    void *w = nullptr, *pl = nullptr;
    int rc = get_scratch(12, sums_b + (size_t)n_stream * sizeof(T), &w);
    if (rc) return rc;
    if (plan_b && (rc = get_scratch(13, plan_b, &pl))) return rc;
    if (plan_b && (ds_->std_plan_key[0] != stream_size || ds_->std_plan_key[1] != chunk || ds_->std_plan_epoch != ds_->scratch_epoch)) {
        // a new geometry: upload its plans once (the copy is from pageable memory: wait before the vectors go)
        std::vector<uint8_t> h(plan_b);
        std::memcpy(h.data(), lv[0].data(), 4 * lv[0].size());
        std::memcpy(h.data() + 4 * lv[0].size(), lv[1].data(), 4 * lv[1].size());
        std::memcpy(h.data() + lv_b, op[0].data(), op[0].size());
        std::memcpy(h.data() + lv_b + op[0].size(), op[1].data(), op[1].size());
        FA_HIP_TRY(hipMemcpyAsync(pl, h.data(), plan_b, hipMemcpyHostToDevice, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        ds_->std_plan_key[0] = stream_size;
        ds_->std_plan_key[1] = chunk;
        ds_->std_plan_epoch = ds_->scratch_epoch;
    }
    const uint8_t* pb = reinterpret_cast<const uint8_t*>(pl);
    StdPlanRef pf{reinterpret_cast<const int2*>(pb), pb + lv_b, (int)(lv[0].size() / 2), (int)op[0].size()};
    StdPlanRef pt{reinterpret_cast<const int2*>(pb + 4 * lv[0].size()), pb + lv_b + op[0].size(), (int)(lv[1].size() / 2),
                  (int)op[1].size()};
    T* sums = reinterpret_cast<T*>(w);
    T* means = reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(w) + sums_b);
    const unsigned grid = (unsigned)(n_stream * cps), fgrid = (unsigned)((n_stream + 255) / 256);
    hipLaunchKernelGGL((stream_chunk_sum_kernel<T, false>), dim3(grid), dim3(64), 0, st, d_in, stream_size, chunk, cps,
                       (const T*)nullptr, pf, pt, sums);
    hipLaunchKernelGGL((stream_fold_kernel<T, false>), dim3(fgrid), dim3(256), 0, st, sums, n_stream, stream_size, cps, means);
    hipLaunchKernelGGL((stream_chunk_sum_kernel<T, true>), dim3(grid), dim3(64), 0, st, d_in, stream_size, chunk, cps,
                       (const T*)means, pf, pt, sums);
    hipLaunchKernelGGL((stream_fold_kernel<T, true>), dim3(fgrid), dim3(256), 0, st, sums, n_stream, stream_size, cps, d_out);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

}  // namespace

extern "C" {

const char* fa_version(void) { return "flacarray_hip 0.1.0 (gfx950)"; }
int fa_abi_version(void) { return FA_ABI_VERSION; }

int fa_set_decode_verify(int on) {
    const bool was = g_verify.exchange(on != 0);
    return was ? 1 : 0;
}

int fa_set_encode_verify(int on) {
    const bool was = on < 0 ? g_encode_verify.load() : g_encode_verify.exchange(on != 0);
    return was ? 1 : 0;
}

int fa_set_encode_md5(int on) {
    const bool was = on < 0 ? g_encode_md5.load() : g_encode_md5.exchange(on != 0);
    return was ? 1 : 0;
}

void fa_profile_enable(int on) { g_prof = (on != 0); }  // process-wide switch; the events are per device

#ifdef FA_STAMPS
// diagnostic build only (-DFA_STAMPS, flacarray_amd/build.py --stamps): read (and optionally clear) the per-phase
// cycle sums of K3.  Not part of the shipped ABI.
int fa_debug_stamps(unsigned long long* out32, int reset) {
    FA_API_LOCK;
    void* sp = nullptr;
    if (get_scratch(6, 512, &sp)) return FA_ERROR_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess) return FA_ERROR_DEVICE;
    if (hipMemcpy(out32, sp, 512, hipMemcpyDeviceToHost) != hipSuccess) return FA_ERROR_DEVICE;
    if (reset && hipMemset(sp, 0, 512) != hipSuccess) return FA_ERROR_DEVICE;
    return FA_ERROR_NONE;
}
#endif

int fa_profile_read(float* ms, int n) {
    FA_API_LOCK;
    for (int k = 0; k < n; ++k) {
        ms[k] = -1.0f;
        if (k < kProfPairs && ds_->ev_ready && ds_->ev_set[k]) {
            if (hipEventSynchronize(ds_->ev[2 * k + 1]) != hipSuccess) return FA_ERROR_DEVICE;
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ds_->ev[2 * k], ds_->ev[2 * k + 1]) == hipSuccess) ms[k] = t;
        }
    }
    return FA_ERROR_NONE;
}

int fa_profile_last(float* ms3) { return fa_profile_read(ms3, 3); }

int fa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void fa_release_scratch(void) {
    FA_API_LOCK_OR(return);
    for (int i = 0; i < kScratchSlots; ++i) {
        if (ds_->scratch[i]) (void)hipFree(ds_->scratch[i]);
        ds_->scratch[i] = nullptr;
        ds_->scratch_bytes[i] = 0;
    }
    ds_->scratch_epoch++;
    if (ds_->pin) (void)hipHostFree(ds_->pin);
    ds_->pin = ds_->pin_dev = nullptr;
    ds_->pin_tried = false;
}

// test-only: make every scratch slot dirty on purpose.  byte in 0..255 fills every held slot over its whole allocation
// and is remembered, so that a slot get_scratch allocates later starts filled too; -1 turns that off again (and fills
// nothing).  Either way the epoch moves on: the header table and the std plans live in slots and are no longer trusted.
int fa_debug_scratch_fill(int byte) {
    if (byte < -1 || byte > 255) return FA_ERROR_ALLOC;
    FA_API_LOCK;
    FA_HIP_TRY(hipDeviceSynchronize());
    ds_->debug_fill = byte;
    if (byte >= 0) {
        for (int i = 0; i < kScratchSlots; ++i)
            if (ds_->scratch[i]) FA_HIP_TRY(hipMemset(ds_->scratch[i], byte, ds_->scratch_bytes[i]));
        FA_HIP_TRY(hipDeviceSynchronize());
    }
    ds_->scratch_epoch++;
    ds_->stamps_zeroed = false;
    return FA_ERROR_NONE;
}

// test-only: out[i] = bytes slot i holds now, for i < min(n, kScratchSlots) (zeros without a device); returns kScratchSlots
int fa_debug_scratch_bytes(int64_t* out, int n) {
    for (int i = 0; i < n && i < kScratchSlots; ++i) out[i] = 0;
    FA_API_LOCK_OR(return kScratchSlots);
    for (int i = 0; i < n && i < kScratchSlots; ++i) out[i] = (int64_t)ds_->scratch_bytes[i];
    return kScratchSlots;
}

static int64_t slot_workspace_for(int64_t n_stream, int64_t stream_size, uint32_t level, int nch) {
    FramePlan fp;
    if (make_frame_plan(n_stream, stream_size, level, nch, &fp) != FA_ERROR_NONE) return -1;
    return (int64_t)slot_layout(fp).total;
}
int64_t fa_encode_workspace_bytes(int64_t n_stream, int64_t stream_size, uint32_t level) { return slot_workspace_for(n_stream, stream_size, level, 1); }
int64_t fa_encode_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level) { return slot_workspace_for(n_stream, stream_size, level, 2); }

// ---- the steps the three encode sequences share ----
// K3's arguments from a plan: geometry, level parameters, both windows, the per-block-size constants, the caller's slots and
// frame sizes.  hdr (frame_header_table) and stamps (stamps_scratch) are the caller's to set.
static int fill_encode_args(const FramePlan& fp, const int32_t* d_data, uint8_t* slots, uint32_t* frame_bytes, int32_t* d_info, EncodeArgs* a) {
    std::memset(a, 0, sizeof *a);
    a->data = d_data; a->n_stream = fp.n_stream; a->stream_size = fp.stream_size; a->nframes = fp.nf;
    a->B = (int32_t)fp.B; a->tail_bs = fp.tail_bs;
    a->max_lpc_order = fp.P.max_lpc_order; a->max_porder = fp.P.max_porder; a->precision = fp.P.qlp_precision;
    int rc = get_window(a->B, &a->win);
    if (rc) return rc;
    rc = get_window(a->tail_bs, &a->win_tail);
    if (rc) return rc;
    a->slots = slots;
    a->slot_stride = fp.slot_stride;
    a->frame_bytes = frame_bytes;
    a->info = reinterpret_cast<FrameInfo*>(d_info);
    a->pmax_full = fp.pmax_full; a->pmax_tail = fp.pmax_tail;
    a->escale_full = fp.escale_full; a->escale_tail = fp.escale_tail;
    return FA_ERROR_NONE;
}

// frame header fields by frame number: tabulated on the host, cached on the device (per-device state; the caller holds api_mu)
static int frame_header_table(DeviceState* ds, const FramePlan& fp, hipStream_t st, const uint4** out) {
    void* dp = nullptr;
    const int B = (int)fp.B, nch = fp.nch;
    const size_t ntab = (size_t)fp.nf * (nch == 2 ? 2 : 1);  // two-channel arrays: a second half with assignment side + right
    int rc = get_scratch(9, ntab * sizeof(uint4) + 256, &dp);
    if (rc) return rc;
    if (ds->c_nf != fp.nf || ds->c_B != B || ds->c_tail != fp.tail_bs || ds->c_nch != nch || ds->c_dp != dp || ds->c_epoch != ds->scratch_epoch) {
        ds->h_hdr.resize(ntab);
        for (int64_t f = 0; f < fp.nf; ++f) {
            ds->h_hdr[(size_t)f] = frame_header_entry((uint64_t)f, (f == fp.nf - 1) ? fp.tail_bs : B, nch);
            if (nch == 2) ds->h_hdr[(size_t)(fp.nf + f)] = frame_header_entry((uint64_t)f, (f == fp.nf - 1) ? fp.tail_bs : B, nch, true);
        }
        FA_HIP_TRY(hipMemcpyAsync(dp, ds->h_hdr.data(), ntab * sizeof(uint4), hipMemcpyHostToDevice, st));
        FA_HIP_TRY(hipStreamSynchronize(st));  // h_hdr is reused by the next call
        ds->c_nf = fp.nf; ds->c_B = B; ds->c_tail = fp.tail_bs; ds->c_nch = nch; ds->c_dp = dp; ds->c_epoch = ds->scratch_epoch;
    }
    *out = reinterpret_cast<const uint4*>(dp);
    return FA_ERROR_NONE;
}

// diagnostic build (-DFA_STAMPS): the per-phase cycle sums' scratch (fa_debug_stamps), null in every other build
static unsigned long long* stamps_scratch(DeviceState* ds) {
#ifdef FA_STAMPS
    void* sp = nullptr;
    if (get_scratch(6, 512, &sp) == 0) {
        if (!ds->stamps_zeroed) { (void)hipMemset(sp, 0, 512); ds->stamps_zeroed = true; }
        return reinterpret_cast<unsigned long long*>(sp);
    }
#else
    (void)ds;
#endif
    return nullptr;
}

// What a single-pass kernel left at +8 of the ticket block: one copy and one stream synchronisation bring the error
// word, K3F's NaN flag and the scanner's total (headers and short frames included) back; a blob that does not fit the
// caller's buffer is FA_ERROR_ALLOC, any other flag FA_ERROR_ENCODE_PROCESS.
struct PublishBack { int32_t err, nan; int64_t total; };
static_assert(sizeof(PublishBack) == 16, "error word at +8, NaN flag at +12, total at +16 of the ticket block");
static int read_publish_back(const FusedArgs& a, hipStream_t st, PublishBack* back) {
    FA_HIP_TRY(hipMemcpyAsync(back, a.err, sizeof *back, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    if (back->err == 1 || (back->err == 0 && back->total > a.capacity)) return FA_ERROR_ALLOC;  // the blob does not fit the caller's buffer
    if (back->err) {
        std::fprintf(stderr, "flacarray_hip: single-pass encode failed (flags %d: 1 = offset outside the buffer, 2 = a frame timed out waiting for its offset, 4 = the scanner timed out)\n", back->err);
        return FA_ERROR_ENCODE_PROCESS;
    }
    return FA_ERROR_NONE;
}

// ---- the slot sequence: K3 into a slot per frame, K4 (sizes -> offsets, one wait for the total), then K5 into the caller's blob ----
static int encode_device_begin(const int32_t* d_data, int nch, int64_t n_stream, int64_t stream_size, uint32_t level,
                               void* d_workspace, int64_t workspace_bytes, int64_t* d_starts, int64_t* d_nbytes,
                               int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    FA_API_LOCK;
    FramePlan fp;
    int rc = make_frame_plan(n_stream, stream_size, level, nch, &fp);
    if (rc) return rc;
    const SlotLayout pl = slot_layout(fp);
    if (!d_workspace || workspace_bytes < (int64_t)pl.total) return FA_ERROR_ALLOC;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    prof_begin(3, st);
    EncodeArgs a;
    rc = fill_encode_args(fp, d_data, reinterpret_cast<uint8_t*>(ws + pl.off_slots), reinterpret_cast<uint32_t*>(ws + pl.off_fbytes), d_info, &a);
    if (rc) return rc;
    rc = frame_header_table(ds_, fp, st, &a.hdr);
    if (rc) return rc;
    a.stamps = stamps_scratch(ds_);
    prof_begin(0, st);
    launch_encode_for(a, nch, fp.F, st);
    prof_end(0, st);
    int64_t* d_foff = reinterpret_cast<int64_t*>(ws + pl.off_foff);
    int64_t* d_snb = reinterpret_cast<int64_t*>(ws + pl.off_snb);
    int64_t* d_total = reinterpret_cast<int64_t*>(ws + pl.off_total);
    hipLaunchKernelGGL(stream_scan_kernel, dim3((unsigned)n_stream), dim3(256), 0, st, a.frame_bytes, fp.nf, d_foff, d_snb);
    hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(1024), 0, st, d_snb, n_stream, d_starts, d_total);
    FA_HIP_TRY(hipMemcpyAsync(d_nbytes, d_snb, (size_t)n_stream * 8, hipMemcpyDeviceToDevice, st));
    FA_HIP_TRY(hipMemcpyAsync(h_total_bytes, d_total, 8, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

int fa_encode_i32_device_begin(const int32_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level,
                               void* d_workspace, int64_t workspace_bytes, int64_t* d_starts, int64_t* d_nbytes,
                               int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    return encode_device_begin(d_data, 1, n_stream, stream_size, level, d_workspace, workspace_bytes, d_starts, d_nbytes,
                               h_total_bytes, d_info, stream);
}

int fa_encode_i64_device_begin(const int64_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level,
                               void* d_workspace, int64_t workspace_bytes, int64_t* d_starts, int64_t* d_nbytes,
                               int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    return encode_device_begin(reinterpret_cast<const int32_t*>(d_data), 2, n_stream, stream_size, level, d_workspace,
                               workspace_bytes, d_starts, d_nbytes, h_total_bytes, d_info, stream);
}

static int encode_device_finish(int nch, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                                const int64_t* d_starts, unsigned char* d_bytes, void* stream) {
    FA_API_LOCK;
    FramePlan fp;
    int rc = make_frame_plan(n_stream, stream_size, level, nch, &fp);
    if (rc) return rc;
    const SlotLayout pl = slot_layout(fp);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    const uint16_t* crc = nullptr;
    rc = get_crc_tab(&crc);
    if (rc) return rc;
    const int64_t* d_foff = reinterpret_cast<const int64_t*>(ws + pl.off_foff);
    launch_write_headers(st, n_stream, d_bytes, d_starts, d_foff, fp.nf, stream_size, (int32_t)fp.B, (int32_t)fp.tail_bs, (int32_t)nch);
    int64_t nblk = (fp.F + 3) / 4;
#ifndef FA_K5_MAXBLK
#define FA_K5_MAXBLK 32768
#endif
    if (nblk > FA_K5_MAXBLK) nblk = FA_K5_MAXBLK;
    prof_begin(1, st);
    launch_compact_frames(st, nblk, reinterpret_cast<const uint8_t*>(ws + pl.off_slots),
                          reinterpret_cast<const uint32_t*>(ws + pl.off_fbytes), d_foff, d_starts, fp.nf, fp.F, crc, d_bytes,
                          fp.slot_stride);
    prof_end(1, st);
    prof_end(3, st);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

int fa_encode_i32_device_finish(int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                                const int64_t* d_starts, unsigned char* d_bytes, void* stream) {
    return encode_device_finish(1, n_stream, stream_size, level, d_workspace, d_starts, d_bytes, stream);
}

int fa_encode_i64_device_finish(int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                                const int64_t* d_starts, unsigned char* d_bytes, void* stream) {
    return encode_device_finish(2, n_stream, stream_size, level, d_workspace, d_starts, d_bytes, stream);
}

// Every valid geometry has a single-pass encoder: K3F (full mono frames of levels 3-8) or K3G (the rest).
int fa_encode_single_pass_supported(int64_t n_stream, int64_t stream_size, uint32_t level) {
    FramePlan fp;
    return (make_frame_plan(n_stream, stream_size, level, 1, &fp) == FA_ERROR_NONE && !slots_forced()) ? 1 : 0;
}

static int64_t capacity_bytes_for(int64_t n_stream, int64_t stream_size, uint32_t level, int nch) {
    FramePlan fp;
    if (make_frame_plan(n_stream, stream_size, level, nch, &fp) != FA_ERROR_NONE) return -1;
    return fp.capacity;  // (the figure of the slot sequence, of K3F and of K3G, whatever their slots)
}
int64_t fa_encode_capacity_bytes(int64_t n_stream, int64_t stream_size, uint32_t level) { return capacity_bytes_for(n_stream, stream_size, level, 1); }
int64_t fa_encode_capacity_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level) { return capacity_bytes_for(n_stream, stream_size, level, 2); }

// The workspace serves whichever sequence the call takes: K3F's, K3G's (also what K3F's geometries take when the rows
// are not 16-byte aligned), or -- FLACARRAY_HIP_SLOTS -- the slot sequence's.  Both single-pass sequences ask their
// caller for this figure, the one the query answers, not for their own share of it: whether a short workspace is
// refused does not depend on the route the call takes.
static int64_t single_pass_need(const FramePlan& fp) {
    int64_t need = (int64_t)placed_layout(fp).total;
    if (fused_geometry(fp)) need = std::max<int64_t>(need, (int64_t)fused_layout(fp).total);
    return need;
}
static int64_t single_pass_workspace_for(int64_t n_stream, int64_t stream_size, uint32_t level, int nch) {
    FramePlan fp;
    if (make_frame_plan(n_stream, stream_size, level, nch, &fp) != FA_ERROR_NONE) return -1;
    return slots_forced() ? (int64_t)slot_layout(fp).total : single_pass_need(fp);
}
int64_t fa_encode_single_pass_workspace_bytes(int64_t n_stream, int64_t stream_size, uint32_t level) {
    return single_pass_workspace_for(n_stream, stream_size, level, 1);
}
int64_t fa_encode_single_pass_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level) {
    return single_pass_workspace_for(n_stream, stream_size, level, 2);
}

// the single-pass sequence: (float32 input: range pre-pass K1a/K1b,) zero the publish words, K3F, stream headers
static int fused_encode_run(const FramePlan& fp, const void* d_data, bool f32, const float* d_quanta, float* d_offsets, float* d_gains,
                            void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                            int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    FA_API_LOCK;
    const FusedLayout pl = fused_layout(fp);
    const int64_t n_stream = fp.n_stream, stream_size = fp.stream_size;
    if (!d_workspace || workspace_bytes < single_pass_need(fp)) return FA_ERROR_ALLOC;
    // The buffer may be smaller than the worst case (every frame VERBATIM): a frame whose offset lies outside it is not
    // written and the call reports FA_ERROR_ALLOC -- the caller gambles on its data's compressibility and retries with
    // fa_encode_capacity_bytes() if it loses.  It must at least hold the stream headers.
    if (!d_bytes || capacity_bytes < n_stream * fp.hb + 64) return FA_ERROR_ALLOC;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    prof_begin(3, st);
    int* d_nanflag = reinterpret_cast<int*>(ws + pl.pub.off_ticket + 12);  // (inside the zeroed region)
    FA_HIP_TRY(hipMemsetAsync(ws + pl.pub.off_zero, 0, pl.pub.zero_bytes, st));
    if (f32) {
        const int64_t cps = (stream_size + kRangeChunk - 1) / kRangeChunk;
        void* pp = nullptr;
        int rcp = get_scratch(10, (size_t)n_stream * (size_t)cps * 8 + 256, &pp);
        if (rcp) return rcp;
        float* pmin = reinterpret_cast<float*>(pp);
        float* pmax = pmin + n_stream * cps;
        prof_begin(5, st);
        hipLaunchKernelGGL(float32_range_kernel, dim3((unsigned)(n_stream * cps)), dim3(256), 0, st, reinterpret_cast<const float*>(d_data),
                           stream_size, cps, pmin, pmax, d_nanflag);
        hipLaunchKernelGGL(float32_params_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, pmin, pmax, n_stream, cps,
                           d_quanta, d_offsets, d_gains);
        prof_end(5, st);
    }
    FusedArgs a;
    std::memset(&a, 0, sizeof a);
    a.data = reinterpret_cast<const int32_t*>(d_data); a.f_offsets = d_offsets; a.f_gains = d_gains; a.n_stream = n_stream; a.stream_size = stream_size; a.nframes = fp.nf; a.total_frames = fp.F;
    a.max_lpc_order = fp.P.max_lpc_order; a.max_porder = fp.P.max_porder; a.precision = fp.P.qlp_precision;
    a.pmax_full = fp.pmax_full;
    a.escale_full = fp.escale_full;
    a.tail_bs = fp.tail_bs;
    const bool tails = (fp.tail_bs != kMaxBlock);
    int rc = get_window(kMaxBlock, &a.win);
    if (rc) return rc;
    rc = get_crc_tab_fused(&a.crc_tab);
    if (rc) return rc;
    rc = frame_header_table(ds_, fp, st, &a.hdr);
    if (rc) return rc;
    a.blob = d_bytes; a.capacity = capacity_bytes; a.hb = fp.hb;
    point_into_publish_block(pl.pub, ws, &a);
    a.info = reinterpret_cast<FrameInfo*>(d_info);
    a.stamps = stamps_scratch(ds_);
    if (tails) {
        // the short last frame of every stream: the slot encoder (one workgroup per stream) writes it to a slot and its
        // size goes into size_pub, so that the scanner places it between its neighbours like any other frame
        EncodeArgs t;
        rc = fill_encode_args(fp, a.data, reinterpret_cast<uint8_t*>(ws + pl.off_tslots), a.frame_bytes, d_info, &t);
        if (rc) return rc;
        t.hdr = a.hdr;
        t.tail_only = 1;
        launch_encode_for(t, 1, n_stream, st);
        launch_fused_tail_publish(st, a.frame_bytes, a.size_pub, n_stream, fp.nf);
    }
    prof_begin(0, st);
    launch_fused_encode(st, a, f32);
    prof_end(0, st);
    // A frame that was dropped (no offset in time, or an offset outside the buffer) leaves frame_abs / off_pub of
    // itself -- and, after a scanner time-out, of every frame behind it -- unwritten: the kernels below would
    // turn those into addresses.  They run only after the error word has come back clean (one stream
    // synchronisation, ~20 us against a 15 ms kernel): on an error nothing else is launched.  Nothing behind this
    // point changes the three words.
    PublishBack back = {0, 0, 0};
    rc = read_publish_back(a, st, &back);
    if (rc) return rc;
    if (tails) {
        // every frame has its offset now: move the short frames from their slots (byte-shifted copy + CRC-16, K5)
        uint32_t* tb = reinterpret_cast<uint32_t*>(ws + pl.off_tbytes);
        int64_t* toff = reinterpret_cast<int64_t*>(ws + pl.off_toff);
        int64_t* tzero = reinterpret_cast<int64_t*>(ws + pl.off_tzero);
        launch_fused_tail_prep(st, a.off_pub, a.frame_bytes, n_stream, fp.nf, a.frame_abs, tb, toff, tzero);
        const uint16_t* crc5 = nullptr;
        rc = get_crc_tab(&crc5);
        if (rc) return rc;
        int64_t nblk = (n_stream + 3) / 4;
        if (nblk > 32768) nblk = 32768;
        launch_compact_frames(st, nblk, reinterpret_cast<const uint8_t*>(ws + pl.off_tslots), tb, toff, tzero, 1, n_stream, crc5, d_bytes, kSlotBytes);
    }
    launch_fused_finish(st, d_bytes, a.frame_abs, a.frame_bytes, n_stream, fp.nf, stream_size, (int32_t)kMaxBlock, (int32_t)fp.tail_bs, 1, fp.hb,
                        d_starts, d_nbytes, a.total);
    prof_end(3, st);
    // No second wait: the error word, the NaN flag and the total are in hand, and what is still queued (a short-frame
    // compaction, the header / index kernel: microseconds) completes in stream order like everything else a caller
    // queues behind this call -- one host wait per encode (0.172 -> 0.157 ms at 4096 frames).
    FA_HIP_TRY(hipGetLastError());
    *h_total_bytes = back.total;
    if (back.nan & 1) return FA_ERROR_NAN_INPUT;
    return FA_ERROR_NONE;
}


// Small arrays of K3F's geometries take K3G too: K3F's sequence is four launches and two host waits (five more launches
// when the streams end in a short frame), K3G's is one launch and one wait, which wins until the frames are many enough
// for K3F's faster frame loop to pay (tools/bench_placed.py).  FLACARRAY_HIP_PLACED_BELOW overrides the frame count.
static bool placed_preferred(const FramePlan& fp) {
    // (tools/kb_crossover_placed.py, whole frames: 512 frames 0.089 against 0.096 ms, 1024 frames 0.104 against 0.099, 2048
    // frames 0.144 against 0.115; streams that end in a short frame add five launches to K3F's side: 3000 frames 0.166 against 0.22)
    int64_t below = (fp.tail_bs == kMaxBlock) ? kPlacedBelowFrames / 4 : kPlacedBelowFrames;
    if (const char* e = std::getenv("FLACARRAY_HIP_PLACED_BELOW")) below = std::atoll(e);
    return fp.F < below;
}

// the single-pass sequence of every geometry K3F does not take: zero the publish words, K3G, stream headers
static int placed_encode_run(const FramePlan& fp, const int32_t* d_data, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes,
                             int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info,
                             void* stream) {
    FA_API_LOCK;
    const PlacedLayout pl = placed_layout(fp);
    if (!d_workspace || workspace_bytes < single_pass_need(fp)) return FA_ERROR_ALLOC;
    if (!d_bytes || capacity_bytes < fp.n_stream * fp.hb + 64) return FA_ERROR_ALLOC;  // (as for K3F: the buffer may gamble, but holds the headers)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    prof_begin(3, st);
    FA_HIP_TRY(hipMemsetAsync(ws + pl.pub.off_zero, 0, pl.pub.zero_bytes, st));
    EncodeArgs a;
    int rc = fill_encode_args(fp, d_data, reinterpret_cast<uint8_t*>(ws + pl.off_slots), reinterpret_cast<uint32_t*>(ws + pl.pub.off_fbytes), d_info, &a);
    if (rc) return rc;
    rc = frame_header_table(ds_, fp, st, &a.hdr);
    if (rc) return rc;
    FusedArgs p;
    std::memset(&p, 0, sizeof p);
    p.n_stream = fp.n_stream; p.stream_size = fp.stream_size; p.nframes = fp.nf; p.total_frames = fp.F;
    p.blob = d_bytes; p.capacity = capacity_bytes; p.hb = fp.hb;
    point_into_publish_block(pl.pub, ws, &p);
    p.info = a.info;
    rc = get_crc_tab(&p.crc_tab);  // (K5's tables: the placement step is K5's per-frame copy)
    if (rc) return rc;
    p.stamps = a.stamps = stamps_scratch(ds_);  // (the frame body's own phases: stamps[0..16], as in the slot kernel)
    if (p.stamps) (void)hipMemsetAsync(p.stamps + 28, 0, 8, st);  // (start time of the call's first workgroup)
    p.starts = d_starts;
    p.nbytes = d_nbytes;
    prof_begin(0, st);
    launch_encode_placed(st, a, p, fp.nch, placed_grid(fp.F));
    prof_end(0, st);
    prof_end(3, st);
    FA_HIP_TRY(hipGetLastError());
    // one wait: the error word and the total (the kernel has written the index and the stream headers itself)
    PublishBack back = {0, 0, 0};
    rc = read_publish_back(p, st, &back);
    if (rc) return rc;
    *h_total_bytes = back.total;
    return FA_ERROR_NONE;
}

// int32 (nch 1) and int64 (nch 2, the two words of a sample as two channels) arrays
static int encode_device(const int32_t* d_data, int nch, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                         int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    FramePlan fp;
    int rc = make_frame_plan(n_stream, stream_size, level, nch, &fp);
    if (rc) return rc;
    if (slots_forced()) {  // diagnostic: the slot sequence into the same caller-provided buffer
        rc = encode_device_begin(d_data, nch, n_stream, stream_size, level, d_workspace, workspace_bytes, d_starts, d_nbytes, h_total_bytes,
                                 d_info, stream);
        if (rc) return rc;
        if (*h_total_bytes > capacity_bytes) return FA_ERROR_ALLOC;
        return encode_device_finish(nch, n_stream, stream_size, level, d_workspace, d_starts, d_bytes, stream);
    }
    // frames K3F does not cover (two channels, short blocks of levels 0-2, streams shorter than two frames, lengths that are
    // not a multiple of 4, unaligned rows): K3G
    if (!fused_geometry(fp) || (reinterpret_cast<uintptr_t>(d_data) & 15) || placed_preferred(fp))
        return placed_encode_run(fp, d_data, d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, d_info,
                                 stream);
    return fused_encode_run(fp, d_data, false, nullptr, nullptr, nullptr, d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts,
                            d_nbytes, h_total_bytes, d_info, stream);
}

int fa_encode_i32_device(const int32_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                         int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    return encode_device(d_data, 1, n_stream, stream_size, level, d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes,
                         h_total_bytes, d_info, stream);
}

int fa_encode_i64_device(const int64_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                         int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info, void* stream) {
    return encode_device(reinterpret_cast<const int32_t*>(d_data), 2, n_stream, stream_size, level, d_workspace, workspace_bytes, d_bytes,
                         capacity_bytes, d_starts, d_nbytes, h_total_bytes, d_info, stream);
}

int fa_encode_f32_device(const float* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, const float* d_quanta,
                         void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes,
                         int64_t* d_starts, int64_t* d_nbytes, float* d_offsets, float* d_gains, int64_t* h_total_bytes,
                         int32_t* d_info, void* stream) {
    FramePlan fp;
    const int rc = make_frame_plan(n_stream, stream_size, level, 1, &fp);
    if (rc && rc != FA_ERROR_ENCODE_PROCESS) return rc;  // (the argument errors come first; a limit is not K3F's geometry, below)
    if (!d_offsets || !d_gains) return FA_ERROR_CONVERT_TYPE;
    // (other geometries: quantise with fa_float32_to_int32_device, then encode the integers)
    if (rc || !fused_geometry(fp, true) || (reinterpret_cast<uintptr_t>(d_data) & 15)) return FA_ERROR_ENCODE_INIT;
    return fused_encode_run(fp, d_data, true, d_quanta, d_offsets, d_gains, d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts,
                            d_nbytes, h_total_bytes, d_info, stream);
}

// ---- append and overwrite (splice_kernels.hpp, K10): span decode, encode of the patched span image, splice --------------
// Both replace the frames [f0, f1) of m streams by the nf_enc frames of a fresh encode of an (m, len) integer image: the
// old samples [lo, hi) of the span with the caller's (m, n) data laid into columns [col, col + n).  Overwrite: the image is
// the span and the data lies inside it.  Append: the span is the old short last frame, the data lies behind it.
// Workspace layout (256-byte aligned regions): the image the encode reads (none when the data is the whole image), the
// decoded old span where it is narrower than the image (append), the participating streams' starts | nbytes, the encode's
// blob (its capacity), its starts | nbytes, the row of every stream in the encode, off_old(f0) | off_old(f1) of every
// stream, the error word and total, and the encode's own workspace.
struct SplicePlan {
    int64_t B, f0, f1, nf_old, nf_new, lo, hi, len, col, nf_enc, size_new, enc_cap, enc_ws;
    bool exact;   // the caller's data is the whole image
    bool append;  // (a negative n_old_bytes is an argument error for overwrite, a stream that does not fit for append)
    size_t off_img, off_stage, off_sub, off_blob, off_idx, off_slot, off_off, off_small, off_ws, total;
};
// The old store's block size and frame count, from the frame plan of its geometry; the plan's argument errors are the
// call's.  (Its limits are not: they were the old store's own encode's to refuse, and the span's encode has its plan below.)
static int splice_old_geometry(int nch, int64_t n_stream, int64_t stream_size, uint32_t level, SplicePlan* pl) {
    FramePlan old;
    const int rc = make_frame_plan(n_stream, stream_size, level, nch, &old);
    if (rc && rc != FA_ERROR_ENCODE_PROCESS) return rc;
    pl->B = old.B;
    pl->nf_old = old.nf;
    return FA_ERROR_NONE;
}
// the rest of a plan whose B, f0, f1, nf_old, lo, hi, len, col and size_new are set
static int finish_splice_plan(int nch, int64_t n_stream, int64_t m, int64_t n, uint32_t level, SplicePlan* pl) {
    FramePlan enc;  // the encode of the (m, len) image
    if (make_frame_plan(m, pl->len, level, nch, &enc) != FA_ERROR_NONE) return FA_ERROR_ENCODE_INIT;
    pl->nf_enc = enc.nf;
    pl->nf_new = pl->f0 + pl->nf_enc + (pl->nf_old - pl->f1);
    pl->exact = (pl->col == 0 && n == pl->len);
    pl->enc_cap = enc.capacity;
    pl->enc_ws = single_pass_workspace_for(m, pl->len, level, nch);
    // the frames behind the span keep their numbers: no suffix, or no change in the frame count
    if (pl->f1 != pl->nf_old && pl->nf_enc != pl->f1 - pl->f0) return FA_ERROR_ENCODE_INIT;
    const size_t elt = 4 * (size_t)nch;
    const bool staged = !pl->exact && pl->hi - pl->lo != pl->len;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    pl->off_img = o; o += pl->exact ? 0 : up((size_t)m * (size_t)pl->len * elt);
    pl->off_stage = o; o += staged ? up((size_t)m * (size_t)(pl->hi - pl->lo) * elt) : 0;
    pl->off_sub = o; o += up((size_t)m * 16);
    pl->off_blob = o; o += up((size_t)pl->enc_cap + 64);
    pl->off_idx = o; o += up((size_t)m * 16);
    pl->off_slot = o; o += up((size_t)n_stream * 4);
    pl->off_off = o; o += up((size_t)n_stream * 16);
    pl->off_small = o; o += 256;
    pl->off_ws = o; o += up((size_t)pl->enc_ws);
    pl->total = o;
    return FA_ERROR_NONE;
}
static int make_append_plan(int nch, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level, SplicePlan* pl) {
    const int rc = splice_old_geometry(nch, n_stream, stream_size, level, pl);
    if (rc) return rc;
    if (n <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    pl->append = true;
    pl->f1 = pl->nf_old;
    pl->f0 = stream_size / pl->B;  // the old full frames are kept
    pl->lo = pl->f0 * pl->B;
    pl->hi = stream_size;
    pl->col = pl->hi - pl->lo;
    pl->len = pl->col + n;
    pl->size_new = stream_size + n;
    return finish_splice_plan(nch, n_stream, n_stream, n, level, pl);
}
static int make_overwrite_plan(int nch, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level, SplicePlan* pl) {
    // (a count of participating streams outside [1, n_stream] is refused where the plan refuses a stream count)
    const int rc = splice_old_geometry(nch, (m > 0 && m <= n_stream) ? n_stream : 0, stream_size, level, pl);
    if (rc) return rc;
    if (n <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    if (first < 0 || first > stream_size || n > stream_size - first) return FA_ERROR_DECODE_SAMPLE_RANGE;
    pl->append = false;
    pl->f0 = first / pl->B;
    pl->f1 = std::min<int64_t>(pl->nf_old, (first + n + pl->B - 1) / pl->B);
    pl->lo = pl->f0 * pl->B;
    pl->hi = std::min<int64_t>(pl->f1 * pl->B, stream_size);
    pl->len = pl->hi - pl->lo;
    pl->col = first - pl->lo;
    pl->size_new = stream_size;
    return finish_splice_plan(nch, n_stream, m, n, level, pl);
}

static int64_t append_workspace_for(int nch, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    SplicePlan pl;
    return make_append_plan(nch, n_stream, stream_size, n, level, &pl) ? -1 : (int64_t)pl.total;
}
static int64_t overwrite_workspace_for(int nch, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level) {
    SplicePlan pl;
    return make_overwrite_plan(nch, n_stream, stream_size, m, first, n, level, &pl) ? -1 : (int64_t)pl.total;
}
// a participating stream grows by at most the bytes of its span's encode plus 6 bytes per renumbered frame (the middle
// frames it loses only make it smaller, and the stream header of the result is never longer than the two it replaces)
static int64_t splice_capacity(const SplicePlan& pl, int64_t n_old_bytes, int64_t m) { return n_old_bytes + pl.enc_cap + 6 * pl.nf_enc * m + 64; }
static int64_t append_capacity_for(int nch, int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    SplicePlan pl;
    return make_append_plan(nch, n_stream, stream_size, n, level, &pl) ? -1 : splice_capacity(pl, n_old_bytes, n_stream);
}
static int64_t overwrite_capacity_for(int nch, int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n,
                                      uint32_t level) {
    SplicePlan pl;
    return make_overwrite_plan(nch, n_stream, stream_size, m, first, n, level, &pl) ? -1 : splice_capacity(pl, n_old_bytes, m);
}

// samples [lo, hi) of m streams into dense rows of `out`; the (m, len) image `img` into a fresh store numbered from 0
static int decode_span(int nch, const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t m,
                       int64_t stream_size, int64_t lo, int64_t hi, void* out, void* stream) {
    return (nch == 2) ? fa_decode_i64_device(d_old, n_old_bytes, d_starts, d_nbytes, m, stream_size, lo, hi, reinterpret_cast<int64_t*>(out), nullptr,
                                             nullptr, nullptr, stream, -1)
                      : fa_decode_i32_device(d_old, n_old_bytes, d_starts, d_nbytes, m, stream_size, lo, hi, reinterpret_cast<int32_t*>(out), nullptr,
                                             nullptr, nullptr, stream, -1);
}
static int encode_image(int nch, const void* img, int64_t m, int64_t len, uint32_t level, void* d_ws, int64_t ws_bytes, unsigned char* blob,
                        int64_t cap, int64_t* e_idx, int64_t* h_total, void* stream) {
    return (nch == 2) ? fa_encode_i64_device(reinterpret_cast<const int64_t*>(img), m, len, level, d_ws, ws_bytes, blob, cap, e_idx, e_idx + m, h_total,
                                             nullptr, stream)
                      : fa_encode_i32_device(reinterpret_cast<const int32_t*>(img), m, len, level, d_ws, ws_bytes, blob, cap, e_idx, e_idx + m, h_total,
                                             nullptr, stream);
}

static int splice_run(int nch, const SplicePlan& pl, const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts,
                      const int64_t* d_old_nbytes, int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const void* d_data,
                      int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes,
                      int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    if (!d_workspace || workspace_bytes < (int64_t)pl.total) return FA_ERROR_ALLOC;
    if (!d_bytes || capacity_bytes <= 0) return FA_ERROR_ALLOC;
    // (the splice reads its sources in aligned 16-byte blocks)
    if ((reinterpret_cast<uintptr_t>(d_old) & 15) || (reinterpret_cast<uintptr_t>(d_workspace) & 15) || !d_data || (!pl.append && n_old_bytes < 0))
        return FA_ERROR_ENCODE_INIT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    const size_t elt = 4 * (size_t)nch;
    // 0. the stream index, and every participating stream one this encoder wrote with the call's block size, channel count
    //    and stream size, its seek offsets of f0 and f1 inside its body
    SpliceArgs a;
    std::memset(&a, 0, sizeof a);
    a.old = d_old; a.old_bytes = n_old_bytes; a.old_starts = d_old_starts; a.old_nbytes = d_old_nbytes;
    a.sidx = d_stream_index;
    a.slot = reinterpret_cast<int32_t*>(ws + pl.off_slot);
    a.sub_starts = reinterpret_cast<int64_t*>(ws + pl.off_sub);
    a.sub_nbytes = a.sub_starts + m;
    a.off0 = reinterpret_cast<int64_t*>(ws + pl.off_off);
    a.off1 = a.off0 + n_stream;
    a.starts = d_starts; a.nbytes = d_nbytes; a.out = d_bytes;
    a.err = reinterpret_cast<int*>(ws + pl.off_small);
    a.n_stream = n_stream; a.m = m; a.size_old = stream_size; a.size_new = pl.size_new;
    a.f0 = pl.f0; a.f1 = pl.f1; a.nf_old = pl.nf_old; a.nf_new = pl.nf_new;
    a.B = (int32_t)pl.B; a.nch = nch;
    FA_HIP_TRY(hipMemsetAsync(ws + pl.off_small, 0, 16, st));
    if (d_stream_index) {
        FA_HIP_TRY(hipMemsetAsync(a.slot, 0xFF, (size_t)n_stream * 4, st));
    }
    hipLaunchKernelGGL(splice_check_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a);
    {
        int h_err = 0;
        FA_HIP_TRY(hipMemcpyAsync(&h_err, a.err, sizeof h_err, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        FA_HIP_TRY(hipGetLastError());
        if (h_err & 4) return FA_ERROR_DECODE_SEEK;
        if (h_err) return FA_ERROR_DECODE_INIT;
    }
    // 1. the image: the old samples of the span, decoded (the existing decoders; through a staging copy where the image is
    //    wider than the span), with the new samples laid into their columns -- or the new samples as they are when they are
    //    the whole image
    char* img = ws + pl.off_img;
    int rc;
    if (!pl.exact) {
        const size_t pitch = (size_t)pl.len * elt, span = (size_t)(pl.hi - pl.lo) * elt;
        char* dec = (span != pitch) ? ws + pl.off_stage : img;
        rc = decode_span(nch, d_old, n_old_bytes, a.sub_starts, a.sub_nbytes, m, stream_size, pl.lo, pl.hi, dec, stream);
        if (rc) return rc;
        if (dec != img) {
            FA_HIP_TRY(hipMemcpy2DAsync(img, pitch, dec, span, span, (size_t)m, hipMemcpyDeviceToDevice, st));
        }
        FA_HIP_TRY(hipMemcpy2DAsync(img + (size_t)pl.col * elt, pitch, d_data, (size_t)n * elt, (size_t)n * elt, (size_t)m, hipMemcpyDeviceToDevice, st));
    } else {
        img = reinterpret_cast<char*>(const_cast<void*>(d_data));
    }
    // 2. encode the image (K3F / K3G / the slot sequence, as for any array): nf_enc frames, numbered from 0
    unsigned char* blob = reinterpret_cast<unsigned char*>(ws + pl.off_blob);
    int64_t* e_idx = reinterpret_cast<int64_t*>(ws + pl.off_idx);
    int64_t enc_total = 0;
    rc = encode_image(nch, img, m, pl.len, level, ws + pl.off_ws, pl.enc_ws, blob, pl.enc_cap, e_idx, &enc_total, stream);
    if (rc) return rc;
    // 3. sizes, starts (one wait: the error word and the total), then the splice
    a.enc = blob; a.enc_bytes = enc_total; a.enc_starts = e_idx; a.enc_nbytes = e_idx + m;
    int64_t* d_total = reinterpret_cast<int64_t*>(ws + pl.off_small + 8);
    FA_HIP_TRY(hipMemsetAsync(ws + pl.off_small, 0, 16, st));
    hipLaunchKernelGGL(splice_size_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(1024), 0, st, d_nbytes, n_stream, d_starts, d_total);
    struct { int32_t err, pad; int64_t total; } back = {0, 0, 0};
    FA_HIP_TRY(hipMemcpyAsync(&back, a.err, sizeof back, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (back.err) return FA_ERROR_DECODE_INIT;  // (the old streams were checked above already; the new encode's index is checked here)
    if (back.total > capacity_bytes) return FA_ERROR_ALLOC;
    // workgroups per stream: ~64 KB of the result each (at most 1024, and a grid of fewer than 2^23 workgroups)
    int64_t parts = std::max<int64_t>(1, std::min<int64_t>(1024, back.total / n_stream / 65536));
    while (parts > 1 && n_stream * parts >= (1LL << 23)) parts >>= 1;
    if (n_stream * parts >= (1LL << 31) / 256) return FA_ERROR_ALLOC;
    a.parts = (int32_t)parts;
    hipLaunchKernelGGL(splice_kernel, dim3((unsigned)(n_stream * parts)), dim3(256), 0, st, a);
    FA_HIP_TRY(hipGetLastError());
    *h_total_bytes = back.total;
    return FA_ERROR_NONE;
}

static int append_run(int nch, const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                      int64_t n_stream, int64_t stream_size, const void* d_data, int64_t n, uint32_t level, void* d_workspace,
                      int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                      int64_t* h_total_bytes, void* stream) {
    FA_API_LOCK;
    SplicePlan pl;
    int rc = make_append_plan(nch, n_stream, stream_size, n, level, &pl);
    if (rc) return rc;
    return splice_run(nch, pl, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, nullptr, n_stream, d_data, n, level, d_workspace,
                      workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}
static int overwrite_run(int nch, const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                         int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const void* d_data, int64_t first,
                         int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes,
                         int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    FA_API_LOCK;
    if (!d_stream_index && m != n_stream) return FA_ERROR_ZERO_NSTREAM;
    SplicePlan pl;
    int rc = make_overwrite_plan(nch, n_stream, stream_size, m, first, n, level, &pl);
    if (rc) return rc;
    return splice_run(nch, pl, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, d_stream_index, m, d_data, n, level, d_workspace,
                      workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}

}  // extern "C" (a template needs C++ linkage)
// fill_ranges_kernel<T> (scrub_kernels.hpp) with the element at fill_value
template <typename T>
static void launch_fill(void* d_out, int64_t n_ranges, const int64_t* d_off, const int64_t* d_count, const void* fill_value, hipStream_t st) {
    T v;
    std::memcpy(&v, fill_value, sizeof(T));
    const unsigned grid = (unsigned)(n_ranges < (int64_t)1 << 20 ? n_ranges : (int64_t)1 << 20);
    hipLaunchKernelGGL((fill_ranges_kernel<T>), dim3(grid), dim3(256), 0, st, reinterpret_cast<T*>(d_out), n_ranges, d_off, d_count, v);
}

template <typename F, typename I>
static int quantise_given_run(const F* d_in, int64_t n_stream, int64_t n, const F* d_offsets, const F* d_gains, I* d_out, int64_t out_stride,
                              void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (n <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    if (!d_in || !d_offsets || !d_gains || !d_out || out_stride < n) return FA_ERROR_CONVERT_TYPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* p = nullptr;
    int rc = get_scratch(4, 256, &p);
    if (rc) return rc;
    int* d_flags = reinterpret_cast<int*>(p);
    FA_HIP_TRY(hipMemsetAsync(d_flags, 0, 4, st));
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(16384, (n_stream * n + 1023) / 1024));
    hipLaunchKernelGGL((quantise_rows_kernel<F, I>), dim3((unsigned)blocks), dim3(256), 0, st, d_in, n_stream, n, d_offsets, d_gains, d_out,
                       out_stride, d_flags);
    int h = 0;
    FA_HIP_TRY(hipMemcpyAsync(&h, d_flags, 4, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    return (h & 1) ? FA_ERROR_NAN_INPUT : FA_ERROR_NONE;
}
extern "C" {

int64_t fa_append_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    return append_workspace_for(1, n_stream, stream_size, n, level);
}
int64_t fa_append_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    return append_workspace_for(2, n_stream, stream_size, n, level);
}
int64_t fa_append_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    return append_capacity_for(1, n_old_bytes, n_stream, stream_size, n, level);
}
int64_t fa_append_capacity_bytes_i64(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level) {
    return append_capacity_for(2, n_old_bytes, n_stream, stream_size, n, level);
}
int fa_append_i32_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                         int64_t n_stream, int64_t stream_size, const int32_t* d_data, int64_t n, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                         int64_t* h_total_bytes, void* stream) {
    return append_run(1, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, d_data, n, level, d_workspace, workspace_bytes,
                      d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}
int fa_append_i64_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                         int64_t n_stream, int64_t stream_size, const int64_t* d_data, int64_t n, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                         int64_t* h_total_bytes, void* stream) {
    return append_run(2, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, d_data, n, level, d_workspace, workspace_bytes,
                      d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}
int fa_quantise_f32_device(const float* d_input, int64_t n_stream, int64_t n, const float* d_offsets, const float* d_gains, int32_t* d_output,
                           int64_t out_stride, void* stream) {
    return quantise_given_run<float, int32_t>(d_input, n_stream, n, d_offsets, d_gains, d_output, out_stride, stream);
}
int fa_quantise_f64_device(const double* d_input, int64_t n_stream, int64_t n, const double* d_offsets, const double* d_gains, int64_t* d_output,
                           int64_t out_stride, void* stream) {
    return quantise_given_run<double, int64_t>(d_input, n_stream, n, d_offsets, d_gains, d_output, out_stride, stream);
}

int64_t fa_overwrite_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level) {
    return overwrite_workspace_for(1, n_stream, stream_size, m, first, n, level);
}
int64_t fa_overwrite_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level) {
    return overwrite_workspace_for(2, n_stream, stream_size, m, first, n, level);
}
int64_t fa_overwrite_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n,
                                    uint32_t level) {
    return overwrite_capacity_for(1, n_old_bytes, n_stream, stream_size, m, first, n, level);
}
int64_t fa_overwrite_capacity_bytes_i64(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n,
                                        uint32_t level) {
    return overwrite_capacity_for(2, n_old_bytes, n_stream, stream_size, m, first, n, level);
}
int fa_overwrite_i32_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                            int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const int32_t* d_data,
                            int64_t first, int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes,
                            int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    return overwrite_run(1, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, d_stream_index, m, d_data, first, n, level,
                         d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}
int fa_overwrite_i64_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                            int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const int64_t* d_data,
                            int64_t first, int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes,
                            int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    return overwrite_run(2, d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, d_stream_index, m, d_data, first, n, level,
                         d_workspace, workspace_bytes, d_bytes, capacity_bytes, d_starts, d_nbytes, h_total_bytes, stream);
}

int fa_decode_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                         const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t first_sample,
                         int64_t last_sample, int32_t* d_out_i32, float* d_out_f32, const float* d_offsets,
                         const float* d_gains, void* stream, int verify) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    int rc = check_output_args(d_out_i32, d_out_f32, d_offsets, d_gains);
    if (rc) return rc;
    DecodeRequest r;
    if ((rc = validate_range(stream_size, first_sample, last_sample, &r.first, &r.n_decode))) return rc;
    r.st = reinterpret_cast<hipStream_t>(stream); r.verify = verify;
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size).output(d_out_i32, d_out_f32, d_offsets, d_gains));
}

int fa_decode_slices_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                                const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t n_slices,
                                const int64_t* slice_stream, const int64_t* slice_first, const int64_t* slice_count,
                                const int64_t* out_offset, int32_t* d_out_i32, float* d_out_f32,
                                const float* d_offsets, const float* d_gains, void* stream, int verify) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (n_slices <= 0) return FA_ERROR_NONE;
    if (const int rc = check_output_args(d_out_i32, d_out_f32, d_offsets, d_gains)) return rc;
    DecodeRequest r;
    r.st = reinterpret_cast<hipStream_t>(stream); r.verify = verify;
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size)
                                  .slices(n_slices, slice_stream, slice_first, slice_count, out_offset)
                                  .output(d_out_i32, d_out_f32, d_offsets, d_gains));
}

int fa_decode_index_create(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                           int64_t n_stream, int64_t stream_size, int channels, void** index, void* stream) {
    FA_API_LOCK;
    if (!index) return FA_ERROR_ALLOC;
    *index = nullptr;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (channels != 1 && channels != 2) return FA_ERROR_CONVERT_TYPE;
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return FA_ERROR_DECODE_INIT;  // (an index refers to the caller's bytes, not to a realigned copy)
    DecodeIndex* ix = new (std::nothrow) DecodeIndex();
    if (!ix) return FA_ERROR_ALLOC;
    (void)hipGetDevice(&ix->device);
    const int rc = build_decode_tables(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, channels, reinterpret_cast<hipStream_t>(stream), true, ix);
    if (rc) {
        if (ix->meta) (void)hipFree(ix->meta);
        if (ix->ftab) (void)hipFree(ix->ftab);
        delete ix;
        return rc;
    }
    *index = ix;
    return FA_ERROR_NONE;
}

void fa_decode_index_destroy(void* index) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return;
    // the index belongs to the device it was created on: free it there, whatever the caller's current device is
    int cur = -1;
    (void)hipGetDevice(&cur);
    const bool hop = (ix->device >= 0 && cur != ix->device);
    if (hop) (void)hipSetDevice(ix->device);
    struct Back { bool on; int dev; ~Back() { if (on) (void)hipSetDevice(dev); } } back{hop, cur};
    FA_API_LOCK_OR(return);
    if (ix->meta) (void)hipFree(ix->meta);
    if (ix->ftab) (void)hipFree(ix->ftab);
    if (ix->tasks) (void)hipFree(ix->tasks);
    delete ix;
}

int fa_decode_indexed(void* index, int64_t first_sample, int64_t last_sample, int64_t n_slices, const int64_t* slice_stream,
                      const int64_t* slice_first, const int64_t* slice_count, const int64_t* out_offset, void* d_out_int,
                      void* d_out_float, const void* d_offsets, const void* d_gains, void* stream, int verify) {
    FA_API_LOCK;
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    int rc;
    if ((rc = index_on_device(ix))) return rc;
    if ((rc = check_output_args(d_out_int, d_out_float, d_offsets, d_gains))) return rc;
    DecodeRequest r;
    if (n_slices < 0) {
        if ((rc = validate_range(ix->stream_size, first_sample, last_sample, &r.first, &r.n_decode))) return rc;
    } else if (n_slices == 0) {
        return FA_ERROR_NONE;
    }
    r.idx = ix; r.nch = ix->nch; r.st = reinterpret_cast<hipStream_t>(stream); r.verify = verify;
    return decode_device_impl(r.slices(n_slices, slice_stream, slice_first, slice_count, out_offset).output(d_out_int, d_out_float, d_offsets, d_gains));
}

void* fa_pinned_alloc(int64_t bytes) {
    if (bytes <= 0 || fa_device_count() <= 0) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void fa_pinned_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int fa_decode_indexed_host(void* index, int64_t n_slices, const int64_t* slice_stream, const int64_t* slice_first,
                           const int64_t* slice_count, const int64_t* out_offset, void* d_out_int, void* d_out_float,
                           const void* d_offsets, const void* d_gains, void* h_out, int64_t out_bytes, void* stream, int verify) {
    FA_API_LOCK;
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix || !h_out || out_bytes < 0) return FA_ERROR_DECODE_INIT;
    int rc;
    if ((rc = index_on_device(ix))) return rc;
    if ((rc = check_output_args(d_out_int, d_out_float, d_offsets, d_gains))) return rc;
    if (n_slices <= 0) return FA_ERROR_NONE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bool copied = false;
    DecodeRequest r;
    r.idx = ix; r.nch = ix->nch; r.st = st; r.verify = verify;
    if (ix->nch == 1) { r.h_copy = h_out; r.h_copy_bytes = (size_t)out_bytes; r.copied = &copied; }  // (the landing is K7L's one-channel route's)
    rc = decode_device_impl(r.slices(n_slices, slice_stream, slice_first, slice_count, out_offset).output(d_out_int, d_out_float, d_offsets, d_gains));
    if (rc) return rc;
    if (!copied && out_bytes > 0) {
        FA_HIP_TRY(hipMemcpyAsync(h_out, d_out_int ? d_out_int : d_out_float, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
    }
    return FA_ERROR_NONE;
}

int fa_decode_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                         const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t first_sample,
                         int64_t last_sample, int64_t* d_out_i64, double* d_out_f64, const double* d_offsets,
                         const double* d_gains, void* stream, int verify) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    int rc = check_output_args(d_out_i64, d_out_f64, d_offsets, d_gains);
    if (rc) return rc;
    DecodeRequest r;
    if ((rc = validate_range(stream_size, first_sample, last_sample, &r.first, &r.n_decode))) return rc;
    r.nch = 2; r.st = reinterpret_cast<hipStream_t>(stream); r.verify = verify;
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size).output(d_out_i64, d_out_f64, d_offsets, d_gains));
}

int fa_decode_slices_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                                const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t n_slices,
                                const int64_t* slice_stream, const int64_t* slice_first, const int64_t* slice_count,
                                const int64_t* out_offset, int64_t* d_out_i64, double* d_out_f64,
                                const double* d_offsets, const double* d_gains, void* stream, int verify) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (n_slices <= 0) return FA_ERROR_NONE;
    if (const int rc = check_output_args(d_out_i64, d_out_f64, d_offsets, d_gains)) return rc;
    DecodeRequest r;
    r.nch = 2; r.st = reinterpret_cast<hipStream_t>(stream); r.verify = verify;
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size)
                                  .slices(n_slices, slice_stream, slice_first, slice_count, out_offset)
                                  .output(d_out_i64, d_out_f64, d_offsets, d_gains));
}

static int compare_device(int nch, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                          int64_t n_stream, int64_t stream_size, const void* d_data, const void* d_offsets, const void* d_gains,
                          int64_t* d_first_mismatch, void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (!d_data || !d_first_mismatch || (d_offsets == nullptr) != (d_gains == nullptr)) return FA_ERROR_CONVERT_TYPE;
    DecodeRequest r;
    r.nch = nch; r.n_decode = stream_size; r.st = reinterpret_cast<hipStream_t>(stream);
    r.offsets = d_offsets; r.gains = d_gains; r.cmp = d_data; r.first_mismatch = d_first_mismatch;  // (the sink forces verify to 0)
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size));
}

int fa_compare_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                          int64_t n_stream, int64_t stream_size, const void* d_data, const float* d_offsets, const float* d_gains,
                          int64_t* d_first_mismatch, void* stream) {
    return compare_device(1, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, d_data, d_offsets, d_gains, d_first_mismatch,
                          stream);
}

int fa_compare_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                          int64_t n_stream, int64_t stream_size, const void* d_data, const double* d_offsets, const double* d_gains,
                          int64_t* d_first_mismatch, void* stream) {
    return compare_device(2, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, d_data, d_offsets, d_gains, d_first_mismatch,
                          stream);
}

// ---- STREAMINFO MD5: hash (K10), sign, check --------------------------------------------------------------------
// kind 0 int32, 1 int64, 2 float32, 3 float64 rows (md5_kernels.hpp); n / row_stride / n_before in samples.  Launches in
// stream order; d_flags (the NaN word, float kinds only) is the caller's to clear and read.
static int md5_launch(int kind, const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const void* d_offsets, const void* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, int* d_flags, hipStream_t st) {
    const int wd = (kind & 1) ? 2 : 1;  // dwords per sample
    const uint32_t* p = reinterpret_cast<const uint32_t*>(d_data);
    const int64_t nd = n * wd, sd = row_stride * wd;
    const uint64_t before = (uint64_t)n_before * 4u * (uint64_t)wd;
    const bool vec = ((reinterpret_cast<uintptr_t>(d_data) & 15) == 0) && (n_stream == 1 || (sd & 3) == 0);
    const dim3 grid((unsigned)((n_stream + 63) / 64)), block(64);
    uint32_t* dig = reinterpret_cast<uint32_t*>(d_digest);
#define FA_MD5_GO(K, U) \
    hipLaunchKernelGGL((md5_rows_kernel<K, U>), grid, block, 0, st, p, n_stream, nd, sd, d_offsets, d_gains, d_state, before, final, d_state, dig, d_flags)
    switch (kind) {
        case 0: if (vec) FA_MD5_GO(0, 4); else FA_MD5_GO(0, 1); break;
        case 1: if (vec) FA_MD5_GO(1, 4); else FA_MD5_GO(1, 2); break;
        case 2: if (vec) FA_MD5_GO(2, 4); else FA_MD5_GO(2, 1); break;
        default: if (vec) FA_MD5_GO(3, 4); else FA_MD5_GO(3, 2); break;
    }
#undef FA_MD5_GO
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

static int md5_device(int wide, const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const void* d_offsets, const void* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    const int per_block = wide ? 8 : 16;  // samples in 64 bytes
    if (n < 0 || n_before < 0 || (n > 0 && !d_data) || row_stride < n || (d_offsets == nullptr) != (d_gains == nullptr)) return FA_ERROR_CONVERT_TYPE;
    if (n_before % per_block != 0 || (!final && n % per_block != 0)) return FA_ERROR_CONVERT_TYPE;  // whole 64-byte blocks before the last call
    if ((final && !d_digest) || ((!final || n_before > 0) && !d_state)) return FA_ERROR_CONVERT_TYPE;
    if ((reinterpret_cast<uintptr_t>(d_digest) & 15) || (reinterpret_cast<uintptr_t>(d_state) & 15)) return FA_ERROR_CONVERT_TYPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int kind = (wide ? 1 : 0) + (d_offsets ? 2 : 0);
    if (!d_offsets) return md5_launch(kind, d_data, n_stream, n, row_stride, nullptr, nullptr, d_state, n_before, final, d_digest, nullptr, st);
    void* p = nullptr;
    int rc = get_scratch(15, 256, &p);
    if (rc) return rc;
    int* d_flags = reinterpret_cast<int*>(p);
    FA_HIP_TRY(hipMemsetAsync(d_flags, 0, 4, st));
    if ((rc = md5_launch(kind, d_data, n_stream, n, row_stride, d_offsets, d_gains, d_state, n_before, final, d_digest, d_flags, st))) return rc;
    int h = 0;
    FA_HIP_TRY(hipMemcpyAsync(&h, d_flags, 4, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    return (h & 1) ? FA_ERROR_NAN_INPUT : FA_ERROR_NONE;
}

int fa_md5_i32_device(const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const float* d_offsets, const float* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, void* stream) {
    return md5_device(0, d_data, n_stream, n, row_stride, d_offsets, d_gains, d_state, n_before, final, d_digest, stream);
}

int fa_md5_i64_device(const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const double* d_offsets, const double* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, void* stream) {
    return md5_device(1, d_data, n_stream, n, row_stride, d_offsets, d_gains, d_state, n_before, final, d_digest, stream);
}

int fa_sign_streams_device(unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, int64_t n_stream, const unsigned char* d_digests,
                           void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (!d_bytes || !d_starts || !d_digests || n_bytes < 0) return FA_ERROR_CONVERT_TYPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* p = nullptr;
    int rc = get_scratch(15, 256, &p);
    if (rc) return rc;
    int* d_flag = reinterpret_cast<int*>(p) + 1;
    FA_HIP_TRY(hipMemsetAsync(d_flag, 0, 4, st));
    hipLaunchKernelGGL(sign_check_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, d_bytes, n_bytes, d_starts, n_stream, d_flag);
    int h = 0;
    FA_HIP_TRY(hipMemcpyAsync(&h, d_flag, 4, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (h) return FA_ERROR_DECODE_INIT;  // (nothing written)
    hipLaunchKernelGGL(sign_streams_kernel, dim3((unsigned)((n_stream * 16 + 255) / 256)), dim3(256), 0, st, d_bytes, d_starts, n_stream, d_digests);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

int fa_check_md5_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                        int64_t stream_size, int channels, int64_t max_temp_bytes, int8_t* d_status, unsigned char* d_digests, void* stream,
                        int verify) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (!d_bytes || !d_starts || !d_nbytes || !d_status || (channels != 1 && channels != 2)) return FA_ERROR_CONVERT_TYPE;
    if (reinterpret_cast<uintptr_t>(d_digests) & 15) return FA_ERROR_CONVERT_TYPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // [15]: flags and counts (256 bytes) | chaining states | digests (when the caller wants none)
    void* p = nullptr;
    int rc = get_scratch(15, 256 + (size_t)n_stream * 32, &p);
    if (rc) return rc;
    int* d_counts = reinterpret_cast<int*>(p) + 2;
    uint32_t* d_state = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(p) + 256);
    unsigned char* d_dig = d_digests ? d_digests : reinterpret_cast<unsigned char*>(d_state + 4 * n_stream);
    FA_HIP_TRY(hipMemsetAsync(d_counts, 0, 8, st));
    const dim3 sgrid((unsigned)((n_stream + 255) / 256));
    hipLaunchKernelGGL(md5_classify_kernel, sgrid, dim3(256), 0, st, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, channels, d_status, d_counts);
    int h_counts[2] = {0, 0};
    FA_HIP_TRY(hipMemcpyAsync(h_counts, d_counts, 8, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (d_digests) FA_HIP_TRY(hipMemsetAsync(d_digests, 0, (size_t)n_stream * 16, st));
    // nothing to decide (and no digest asked for that a decode could give): the store is not decoded
    if (h_counts[0] == 0 && !(d_digests && h_counts[1] > 0)) return FA_ERROR_NONE;
    // column chunks: whole 64-byte blocks of every stream, the decoded chunk under the cap
    const int64_t per_block = channels == 2 ? 8 : 16;
    const int64_t sample_bytes = 4 * channels;
    const int64_t cap = max_temp_bytes > 0 ? max_temp_bytes : (int64_t)FA_MD5_CHECK_TEMP_BYTES;
    int64_t width = cap / (n_stream * sample_bytes) / per_block * per_block;
    if (width < per_block) width = per_block;
    if (width > stream_size) width = stream_size;
    void* d_tmp = nullptr;
    if ((rc = get_scratch(14, (size_t)n_stream * (size_t)width * (size_t)sample_bytes + 256, &d_tmp))) return rc;
    for (int64_t at = 0; at < stream_size; at += width) {
        const int64_t w = std::min(width, stream_size - at);
        const bool whole = (w == stream_size);
        const int64_t first = whole ? -1 : at, last = whole ? -1 : at + w;
        rc = channels == 2 ? fa_decode_i64_device(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last,
                                                  reinterpret_cast<int64_t*>(d_tmp), nullptr, nullptr, nullptr, stream, verify)
                           : fa_decode_i32_device(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last,
                                                  reinterpret_cast<int32_t*>(d_tmp), nullptr, nullptr, nullptr, stream, verify);
        if (rc) return rc;
        if ((rc = md5_launch(channels == 2 ? 1 : 0, d_tmp, n_stream, w, w, nullptr, nullptr, d_state, at, at + w == stream_size, d_dig, nullptr, st)))
            return rc;
    }
    hipLaunchKernelGGL(md5_compare_kernel, sgrid, dim3(256), 0, st, d_bytes, d_starts, n_stream, d_dig, d_status);
    FA_HIP_TRY(hipStreamSynchronize(st));  // (the scratch is free again, d_status / d_digests are complete)
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

// ---- binned reduction: min / max / sums of the decoded samples, without a decoded copy -----------------------------
// One-channel streams: the reducing sink of K7, at every width (profiles/reduce.md).  Two-channel streams: decoded column
// chunks of whole frames under a cap, each folded into the bins by the chunk reducers.
// The block size stream 0's STREAMINFO states (minimum = maximum).  Lenient (the two-channel reducers cut their chunks
// at frame boundaries with it): a header that does not say, or says less than 16, costs speed only -- 4096.  Strict (a
// search sizes the caller's arrays by the answer): STREAMINFO is the first metadata block, and a header that does not say
// is FA_ERROR_DECODE_INIT.
static int peek_blocksize(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, hipStream_t st, bool strict, int64_t* B) {
    const int miss = strict ? FA_ERROR_DECODE_INIT : FA_ERROR_NONE;
    if (!strict) *B = 4096;
    int64_t s0 = -1;
    FA_HIP_TRY(hipMemcpyAsync(&s0, d_starts, 8, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    if (s0 < 0 || s0 + 12 > n_bytes) return miss;
    unsigned char h[12];
    FA_HIP_TRY(hipMemcpyAsync(h, d_bytes + s0, 12, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    const int64_t bmin = ((int64_t)h[8] << 8) | h[9], bmax = ((int64_t)h[10] << 8) | h[11];
    if (std::memcmp(h, "fLaC", 4) != 0 || bmin != bmax) return miss;
    if (strict ? ((h[4] & 0x7f) != 0 || bmin <= 0 || bmin > 65535) : bmin < 16) return miss;
    *B = bmin;
    return FA_ERROR_NONE;
}

// What the reducing calls (fa_reduce_*, fa_histogram_*) share: the store named by an index or by its three arrays, the
// sample range (both ends negative: everything)
static int reduce_store_args(int nch, DecodeIndex* ix, const unsigned char*& d_bytes, int64_t& n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                             int64_t& n_stream, int64_t& stream_size, int64_t& first, int64_t& last) {
    if (ix) {
        if (const int rc = index_on_device(ix)) return rc;
        if (ix->nch != nch) return FA_ERROR_DECODE_INIT;
        n_stream = ix->n_stream; stream_size = ix->stream_size; d_bytes = ix->bytes; n_bytes = ix->n_bytes;
    } else if (!d_bytes || !d_starts || !d_nbytes) {
        return FA_ERROR_CONVERT_TYPE;
    }
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (first < 0 && last < 0) { first = 0; last = stream_size; }
    if (first < 0 || last > stream_size || first >= last) return FA_ERROR_DECODE_SAMPLE_RANGE;
    return FA_ERROR_NONE;
}

// Two-channel stores: [first, last) of the rows (all streams, or the `rows` streams d_sel names) decoded in column chunks
// of whole frames under the cap; fold(chunk, at, end) launches what folds the int64 chunk [rows][end - at] of samples
// [at, end) into the caller's arrays, on `st`.
static int reduce_chunks(DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                         int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t rows, const int64_t* d_sel,
                         int64_t max_temp_bytes, hipStream_t st, int verify,
                         const std::function<int(const long long*, int64_t, int64_t)>& fold, int64_t B_known = 0) {
    const int64_t n = last - first;
    int rc;
    int64_t B = ix ? ix->B : B_known;
    if (B <= 0 && (rc = peek_blocksize(d_bytes, n_bytes, d_starts, st, false, &B))) return rc;
    const int64_t sample_bytes = 8;
    const int64_t cap = max_temp_bytes > 0 ? max_temp_bytes : (int64_t)FA_REDUCE_TEMP_BYTES;
    int64_t cw = cap / (rows * sample_bytes) / B * B;
    if (cw < B) cw = B;
    void* d_tmp = nullptr;
    if ((rc = get_scratch(16, (size_t)rows * (size_t)std::min(cw, n) * (size_t)sample_bytes + 256, &d_tmp))) return rc;
    std::vector<int64_t> sl;  // named streams: the chunk as one slice per row (host arrays: stream | first | count | output offset)
    if (d_sel) {
        sl.resize(4 * (size_t)rows);
        FA_HIP_TRY(hipMemcpyAsync(sl.data(), d_sel, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
    }
    DecodeRequest rq;
    rq.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size);
    rq.idx = ix; rq.nch = 2; rq.st = st; rq.verify = verify; rq.out_int = d_tmp;
    if (d_sel) rq.slices(rows, sl.data(), sl.data() + rows, sl.data() + 2 * rows, sl.data() + 3 * rows);
    for (int64_t at = first; at < last;) {
        const int64_t end = std::min(last, at / B * B + cw);  // (chunks after the first start at a frame)
        const int64_t w = end - at;
        if (d_sel)
            for (int64_t r = 0; r < rows; ++r) { sl[rows + r] = at; sl[2 * rows + r] = w; sl[3 * rows + r] = r * w; }
        rq.first = at; rq.n_decode = w;
        if ((rc = decode_device_impl(rq))) return rc;
        if ((rc = fold(reinterpret_cast<const long long*>(d_tmp), at, end))) return rc;
        at = end;
    }
    FA_HIP_TRY(hipStreamSynchronize(st));  // (the scratch is free again, the bins are complete)
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

// One-channel stores: [first, last) through K7 into the sink
static int fold_device(DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                       int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, hipStream_t st, int verify, const FoldSink& sink) {
    DecodeRequest r;
    r.idx = ix; r.first = first; r.n_decode = last - first; r.st = st; r.verify = verify; r.fold = &sink;
    return decode_device_impl(r.store(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size));
}

static int reduce_device(int nch,DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                         int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t width, int64_t n_sel,
                         const int64_t* d_sel, int64_t max_temp_bytes, int64_t* d_min, int64_t* d_max, int64_t* d_sum, uint64_t* d_sq_hi,
                         uint64_t* d_sq_lo, void* stream, int verify) {
    FA_API_LOCK;
    int rc;
    if ((rc = reduce_store_args(nch, ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last))) return rc;
    if (width < 1 || !d_min || !d_max || !d_sum || (d_sq_hi == nullptr) != (d_sq_lo == nullptr) || (nch == 2 && d_sq_hi)) return FA_ERROR_CONVERT_TYPE;
    if (d_sel && n_sel <= 0) return n_sel == 0 ? FA_ERROR_NONE : FA_ERROR_CONVERT_TYPE;
    const int64_t n = last - first;
    if (width > n) width = n;
    const int64_t nbins = (n + width - 1) / width;
    const int64_t rows = d_sel ? n_sel : n_stream;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FoldSink sink;
    sink.kind = FoldSink::kReduce; sink.n_sel = n_sel; sink.sel = d_sel; sink.red.width = width;
    ReduceOut& out = sink.red.out;
    out.mn = reinterpret_cast<long long*>(d_min); out.mx = reinterpret_cast<long long*>(d_max); out.sum = reinterpret_cast<long long*>(d_sum);
    out.sq_hi = reinterpret_cast<unsigned long long*>(d_sq_hi); out.sq_lo = reinterpret_cast<unsigned long long*>(d_sq_lo);
    out.nbins = nbins;
    const int64_t cells = rows * nbins;
    if ((cells + 255) / 256 > 0x7fffffff) return FA_ERROR_ALLOC;
    hipLaunchKernelGGL(reduce_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, out, cells);
    if (nch == 1) return fold_device(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, st, verify, sink);
    return reduce_chunks(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, rows, d_sel, max_temp_bytes, st, verify,
                         [&](const long long* tmp, int64_t at, int64_t end) -> int {
        const int64_t w = end - at;
        if (width >= 64) {
            const int64_t nseg = (w + kReduceSeg - 1) / kReduceSeg;
            if (rows * nseg > 0x7fffffff) return FA_ERROR_ALLOC;
            const dim3 grid((unsigned)(rows * nseg)), block(64);
            hipLaunchKernelGGL(reduce_wave_kernel, grid, block, 0, st, tmp, w, at, first, last, width, nseg, out);
        } else {
            const int64_t bin_lo = (at - first) / width, n_bin = (end - 1 - first) / width - bin_lo + 1;
            const int64_t nblk = (n_bin + 255) / 256;
            if (rows * nblk > 0x7fffffff) return FA_ERROR_ALLOC;
            const dim3 grid((unsigned)(rows * nblk)), block(256);
            hipLaunchKernelGGL(reduce_lane_kernel, grid, block, 0, st, tmp, w, at, first, last, width, bin_lo, n_bin, nblk, out);
        }
        return FA_ERROR_NONE;
    });
}

int fa_reduce_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                         int64_t stream_size, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams,
                         int64_t* d_min, int64_t* d_max, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify) {
    return reduce_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, width, n_sel, d_sel_streams, 0, d_min,
                         d_max, d_sum, d_sq_hi, d_sq_lo, stream, verify);
}

int fa_reduce_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                         int64_t stream_size, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams,
                         int64_t max_temp_bytes, int64_t* d_min, int64_t* d_max, int64_t* d_sum, void* stream, int verify) {
    return reduce_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, width, n_sel, d_sel_streams,
                         max_temp_bytes, d_min, d_max, d_sum, nullptr, nullptr, stream, verify);
}

int fa_reduce_indexed(void* index, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                      int64_t* d_min, int64_t* d_max, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return reduce_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, width, n_sel, d_sel_streams, max_temp_bytes, d_min, d_max,
                         d_sum, d_sq_hi, d_sq_lo, stream, verify);
}

// ---- fold across streams: per-sample sums over groups of streams, without a decoded copy (profiles/common_mode.md) -----
// One-channel streams: the cross-stream sink of K7 (K7X), a wave per (plan row, frame).  Two-channel streams: the column
// chunks of the binned reduction, each summed by xsum_chunk_kernel.  The result arrays are zero-filled here, behind every
// refusal of the arguments: a refused call has written nothing.
static int xsum_device(int nch, DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                       int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                       const int64_t* d_rows, int64_t n_groups, int64_t max_temp_bytes, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo,
                       void* stream, int verify) {
    FA_API_LOCK;
    int rc;
    if ((rc = reduce_store_args(nch, ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last))) return rc;
    if (!d_sum || (d_sq_hi == nullptr) != (d_sq_lo == nullptr) || (nch == 2 && d_sq_hi)) return FA_ERROR_CONVERT_TYPE;
    if (n_groups < 1 || n_sel < 0 || n_rows < 0 || n_sel > n_stream || n_rows > n_sel || (n_sel > 0 && (!d_order || !d_rows || n_rows < 1)))
        return FA_ERROR_CONVERT_TYPE;
    const int64_t n = last - first;
    if (n_groups > INT64_MAX / 8 / n) return FA_ERROR_ALLOC;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t cells_b = (size_t)n_groups * (size_t)n * 8;
#if !(FA_XSUM_MUTANT & 16)
    FA_HIP_TRY(hipMemsetAsync(d_sum, 0, cells_b, st));
    if (d_sq_hi) {
        FA_HIP_TRY(hipMemsetAsync(d_sq_hi, 0, cells_b, st));
        FA_HIP_TRY(hipMemsetAsync(d_sq_lo, 0, cells_b, st));
    }
#else
    (void)cells_b;
#endif
    if (n_sel == 0) return FA_ERROR_NONE;  // (every group is empty)
    if (nch == 1) {
        FoldSink sink;
        sink.kind = FoldSink::kXsum; sink.n_sel = n_sel; sink.sel = d_order;
        sink.xsum.n_rows = n_rows; sink.xsum.rows = d_rows; sink.xsum.n_groups = n_groups;
        sink.xsum.sum = reinterpret_cast<long long*>(d_sum);
        sink.xsum.sq_hi = reinterpret_cast<unsigned long long*>(d_sq_hi); sink.xsum.sq_lo = reinterpret_cast<unsigned long long*>(d_sq_lo);
        return fold_device(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, st, verify, sink);
    }
    return reduce_chunks(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, max_temp_bytes, st, verify,
                         [&](const long long* tmp, int64_t at, int64_t end) -> int {
        const int64_t w = end - at;
        if ((w + 255) / 256 > 0x7fffffff) return FA_ERROR_ALLOC;
        const dim3 grid((unsigned)((w + 255) / 256), (unsigned)std::min<int64_t>(n_groups, 65535)), block(256);
        hipLaunchKernelGGL(xsum_chunk_kernel, grid, block, 0, st, tmp, w, at, first, n, n_sel, d_rows, n_rows, n_groups,
                           reinterpret_cast<long long*>(d_sum));
        return FA_ERROR_NONE;
    });
}

int fa_xsum_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                       const int64_t* d_rows, int64_t n_groups, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify) {
    return xsum_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, n_rows, d_rows, n_groups,
                       0, d_sum, d_sq_hi, d_sq_lo, stream, verify);
}

int fa_xsum_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                       const int64_t* d_rows, int64_t n_groups, int64_t max_temp_bytes, int64_t* d_sum, void* stream, int verify) {
    return xsum_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, n_rows, d_rows, n_groups,
                       max_temp_bytes, d_sum, nullptr, nullptr, stream, verify);
}

int fa_xsum_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows, const int64_t* d_rows,
                    int64_t n_groups, int64_t max_temp_bytes, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return xsum_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, n_sel, d_order, n_rows, d_rows, n_groups, max_temp_bytes, d_sum,
                       d_sq_hi, d_sq_lo, stream, verify);
}

// ---- projections: exact inner products of every row with K templates, without a decoded copy (profiles/dot.md) --------
// One-channel streams: the dot sink of K7 (K7D), kDotKT templates per decode of the range.  Two-channel streams: the
// column chunks of the binned reduction, each folded by dot_chunk_kernel.  The result arrays are zero-filled here, behind
// every refusal of the arguments: a refused call has written nothing.
static int dot_device(int nch, DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                      int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                      const int64_t* d_rows, int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t max_temp_bytes, int64_t* d_hi, uint64_t* d_lo,
                      int64_t* d_out4, void* stream, int verify) {
    FA_API_LOCK;
    int rc;
    if ((rc = reduce_store_args(nch, ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last))) return rc;
    if (!d_tmpl || (nch == 1 ? (!d_hi || !d_lo) : !d_out4)) return FA_ERROR_CONVERT_TYPE;
    if (n_sel < 0 || n_rows < 0 || n_sel > n_stream || n_rows != (n_sel + 63) / 64 || (n_sel > 0 && (!d_order || !d_rows))) return FA_ERROR_CONVERT_TYPE;
    const int64_t n = last - first;
    // (n <= 2^32 - 1: the lower limb of a cell sums n terms below 2^32)
    if (n > 0xffffffffll || K < 1 || ld < K || (ld & 7) != 0) return FA_ERROR_DECODE_SAMPLE_RANGE;
    if (n_sel == 0) return FA_ERROR_NONE;  // (no rows)
    if (K > INT64_MAX / 32 / n_sel) return FA_ERROR_ALLOC;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t cells_b = (size_t)n_sel * (size_t)K * 8;
    if (nch == 1) {
        FA_HIP_TRY(hipMemsetAsync(d_hi, 0, cells_b, st));
        FA_HIP_TRY(hipMemsetAsync(d_lo, 0, cells_b, st));
        FoldSink sink;
        sink.kind = FoldSink::kDot; sink.n_sel = n_sel; sink.sel = d_order;
        sink.dot.n_rows = n_rows; sink.dot.rows = d_rows; sink.dot.K = K; sink.dot.ld = ld; sink.dot.tmpl = d_tmpl;
        sink.dot.hi = reinterpret_cast<unsigned long long*>(d_hi); sink.dot.lo = reinterpret_cast<unsigned long long*>(d_lo);
        // K > kDotKT: one decode of the range per kDotKT templates (the frame CRC-16 check rides with the first)
        for (int64_t k0 = 0; k0 < K; k0 += kDotKT) {
#if (FA_DOT_MUTANT & 8)
            sink.dot.k0 = 0;
#else
            sink.dot.k0 = k0;
#endif
            if ((rc = fold_device(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, st, k0 == 0 ? verify : 0, sink)))
                return rc;
        }
        return FA_ERROR_NONE;
    }
    FA_HIP_TRY(hipMemsetAsync(d_out4, 0, cells_b * 4, st));
    return reduce_chunks(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, max_temp_bytes, st, verify,
                         [&](const long long* tmp, int64_t at, int64_t end) -> int {
        const int64_t w = end - at;
        const int64_t nseg = (w + kReduceSeg - 1) / kReduceSeg;
        if (n_sel * nseg > 0x7fffffff) return FA_ERROR_ALLOC;
        hipLaunchKernelGGL(dot_chunk_kernel, dim3((unsigned)(n_sel * nseg)), dim3(64), 0, st, tmp, w, at, first, nseg, d_tmpl, K, ld,
                           reinterpret_cast<unsigned long long*>(d_out4));
        return FA_ERROR_NONE;
    });
}

int fa_dot_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                      int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                      const int64_t* d_rows, int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t* d_hi, uint64_t* d_lo, void* stream, int verify) {
    return dot_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, n_rows, d_rows, K, ld,
                      d_tmpl, 0, d_hi, d_lo, nullptr, stream, verify);
}

int fa_dot_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                      int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                      const int64_t* d_rows, int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t max_temp_bytes, int64_t* d_out4, void* stream,
                      int verify) {
    return dot_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_order, n_rows, d_rows, K, ld,
                      d_tmpl, max_temp_bytes, nullptr, nullptr, d_out4, stream, verify);
}

int fa_dot_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows, const int64_t* d_rows,
                   int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t max_temp_bytes, int64_t* d_hi, uint64_t* d_lo, int64_t* d_out4,
                   void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return dot_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, n_sel, d_order, n_rows, d_rows, K, ld, d_tmpl, max_temp_bytes,
                      d_hi, d_lo, d_out4, stream, verify);
}

// ---- value histogram: counts per value bin of every row, without a decoded copy (profiles/histogram.md) ----------------
// One-channel streams: the histogram sink of K7 (K7H).  Two-channel streams: the column chunks of the binned reduction,
// each counted by hist_wave_kernel.
static int histogram_device(int nch, DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                            int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel,
                            int64_t max_temp_bytes, int64_t nbins, const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below,
                            int64_t* d_above, void* stream, int verify) {
    FA_API_LOCK;
    int rc;
    if ((rc = reduce_store_args(nch, ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last))) return rc;
    if (nbins < 1 || nbins > kHistMaxBins || !d_lo || !d_shift || !d_counts || !d_below || !d_above) return FA_ERROR_CONVERT_TYPE;
    if (d_sel && n_sel <= 0) return n_sel == 0 ? FA_ERROR_NONE : FA_ERROR_CONVERT_TYPE;
    const int64_t rows = d_sel ? n_sel : n_stream;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HistOut ho;
    ho.counts = reinterpret_cast<unsigned long long*>(d_counts); ho.below = reinterpret_cast<unsigned long long*>(d_below);
    ho.above = reinterpret_cast<unsigned long long*>(d_above);
    ho.lo = reinterpret_cast<const long long*>(d_lo); ho.shift = d_shift; ho.nbins = nbins;
    const int64_t cells = rows * nbins;
    if ((cells + 255) / 256 > 0x7fffffff) return FA_ERROR_ALLOC;
    hipLaunchKernelGGL(hist_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, ho, rows);
    if (nch == 1) {
        FoldSink sink;
        sink.kind = FoldSink::kHist; sink.n_sel = n_sel; sink.sel = d_sel; sink.hist = ho;
        return fold_device(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, st, verify, sink);
    }
    return reduce_chunks(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, rows, d_sel, max_temp_bytes, st, verify,
                         [&](const long long* tmp, int64_t at, int64_t end) -> int {
        const int64_t w = end - at;
        const int64_t nseg = (w + kReduceSeg - 1) / kReduceSeg;
        if (rows * nseg > 0x7fffffff) return FA_ERROR_ALLOC;
        hipLaunchKernelGGL(hist_wave_kernel, dim3((unsigned)(rows * nseg)), dim3(64), 0, st, tmp, w, nseg, ho);
        return FA_ERROR_NONE;
    });
}

int fa_histogram_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t nbins,
                            const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above, void* stream,
                            int verify) {
    return histogram_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, 0, nbins, d_lo,
                            d_shift, d_counts, d_below, d_above, stream, verify);
}

int fa_histogram_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                            int64_t nbins, const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above,
                            void* stream, int verify) {
    return histogram_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, max_temp_bytes,
                            nbins, d_lo, d_shift, d_counts, d_below, d_above, stream, verify);
}

int fa_histogram_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes, int64_t nbins,
                         const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above, void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return histogram_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, n_sel, d_sel_streams, max_temp_bytes, nbins, d_lo, d_shift,
                            d_counts, d_below, d_above, stream, verify);
}

// ---- search: the positions (and values) of the samples outside per-row limits, without a decoded copy (profiles/find.md) ----
// Two passes over the same frames.  Count: hits per (row, frame) into the caller's frame_counts.  Fill: after the caller
// has formed the exclusive prefix sum and listed the cells with a hit, those frames alone are decoded again and their
// hits written in place.  One-channel streams: the search sink of K7 (K7F).  Two-channel streams: the column chunks of
// the binned reduction, counted and filled by the find_chunk kernels -- both passes decode every chunk.

// The block size a search plans with: the index's, or the one stream 0's STREAMINFO states (minimum = maximum, the first
// metadata block).  A header that does not say is an error here: the caller sizes its arrays by the answer.
static int find_blocksize(DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, hipStream_t st, int64_t* B) {
    if (ix) { *B = ix->B; return ix->B > 0 ? FA_ERROR_NONE : FA_ERROR_DECODE_INIT; }
    return peek_blocksize(d_bytes, n_bytes, d_starts, st, true, B);
}

static int find_plan(DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, int64_t stream_size, int64_t first,
                     int64_t last, int64_t* block_size, int64_t* n_frames, void* stream) {
    FA_API_LOCK;
    if (!block_size || !n_frames) return FA_ERROR_CONVERT_TYPE;
    if (ix) {
        if (const int rc = index_on_device(ix)) return rc;
        stream_size = ix->stream_size;
    } else if (!d_bytes || !d_starts) {
        return FA_ERROR_CONVERT_TYPE;
    }
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (first < 0 && last < 0) { first = 0; last = stream_size; }
    if (first < 0 || last > stream_size || first >= last) return FA_ERROR_DECODE_SAMPLE_RANGE;
    int rc;
    int64_t B = 0;
    if ((rc = find_blocksize(ix, d_bytes, n_bytes, d_starts, reinterpret_cast<hipStream_t>(stream), &B))) return rc;
    *block_size = B;
    *n_frames = (last - 1) / B - first / B + 1;
    return FA_ERROR_NONE;
}

int fa_find_plan_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, int64_t stream_size, int64_t first, int64_t last,
                        int64_t* block_size, int64_t* n_frames, void* stream) {
    return find_plan(nullptr, d_bytes, n_bytes, d_starts, stream_size, first, last, block_size, n_frames, stream);
}

int fa_find_plan_indexed(void* index, int64_t first, int64_t last, int64_t* block_size, int64_t* n_frames) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return find_plan(ix, nullptr, 0, nullptr, 0, first, last, block_size, n_frames, nullptr);
}

// fill == false: the count pass (d_frame_counts); fill == true: the fill pass (the hit list, the prefix sum, d_pos, d_val)
static int find_device(int nch, DecodeIndex* ix, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                       int64_t n_stream, int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel,
                       int64_t max_temp_bytes, const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts,
                       bool fill, int64_t n_hit, const int64_t* d_hit, const int64_t* d_offs, int64_t* d_pos, int64_t* d_val, void* stream,
                       int verify) {
    FA_API_LOCK;
    int rc;
    if ((rc = reduce_store_args(nch, ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last))) return rc;
    if (!d_lo || !d_hi || n_frames < 1) return FA_ERROR_CONVERT_TYPE;
    if (fill ? (n_hit < 0 || !d_offs || (n_hit > 0 && (!d_hit || !d_pos))) : !d_frame_counts) return FA_ERROR_CONVERT_TYPE;
    if (d_sel && n_sel <= 0) return n_sel == 0 ? FA_ERROR_NONE : FA_ERROR_CONVERT_TYPE;
    if (fill && n_hit == 0) return FA_ERROR_NONE;
    const int64_t rows = d_sel ? n_sel : n_stream;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FindSink fs;
    fs.lo = reinterpret_cast<const long long*>(d_lo); fs.hi = reinterpret_cast<const long long*>(d_hi); fs.inside = inside ? 1 : 0;
    fs.n_frames = n_frames; fs.frame_counts = reinterpret_cast<long long*>(d_frame_counts);
    fs.n_hit = fill ? n_hit : 0; fs.hit_ids = fill ? reinterpret_cast<const long long*>(d_hit) : nullptr;
    fs.offs = reinterpret_cast<const long long*>(d_offs); fs.pos = reinterpret_cast<long long*>(d_pos); fs.val = reinterpret_cast<long long*>(d_val);
    if (nch == 1) {
        FoldSink sink;
        sink.kind = fill ? FoldSink::kFindFill : FoldSink::kFindCount; sink.n_sel = n_sel; sink.sel = d_sel; sink.find = fs;
        return fold_device(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, st, verify, sink);
    }
    int64_t B = 0;
    if ((rc = find_blocksize(ix, d_bytes, n_bytes, d_starts, st, &B))) return rc;
    const int64_t f0 = first / B, nfr = (last - 1) / B - f0 + 1;
    if (n_frames != nfr) return FA_ERROR_CONVERT_TYPE;
    const int64_t cells = rows * nfr;
    if ((cells + 255) / 256 > 0x7fffffff) return FA_ERROR_ALLOC;
    if (!fill && (rc = find_zero_counts(fs, cells, st))) return rc;
    return reduce_chunks(ix, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, rows, d_sel, max_temp_bytes, st, verify,
                         [&](const long long* tmp, int64_t at, int64_t end) -> int {
        FindChunk c;
        c.data = tmp; c.cw = end - at; c.c0 = at; c.nseg = (end - 1) / B - at / B + 1; c.B = B; c.nfr = nfr; c.f0 = f0;
        c.lo = fs.lo; c.hi = fs.hi; c.inside = fs.inside;
        if (rows * c.nseg > 0x7fffffff) return FA_ERROR_ALLOC;
        if (fill) hipLaunchKernelGGL(find_chunk_fill_kernel, dim3((unsigned)(rows * c.nseg)), dim3(64), 0, st, c, fs.offs, fs.pos, fs.val);
        else hipLaunchKernelGGL(find_chunk_count_kernel, dim3((unsigned)(rows * c.nseg)), dim3(64), 0, st, c, fs.frame_counts);
        return FA_ERROR_NONE;
    }, B);
}

int fa_find_count_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                             int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, const int64_t* d_lo,
                             const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream, int verify) {
    return find_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, 0, d_lo, d_hi,
                       inside, n_frames, d_frame_counts, false, 0, nullptr, nullptr, nullptr, nullptr, stream, verify);
}

int fa_find_count_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                             int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                             const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream,
                             int verify) {
    return find_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, max_temp_bytes,
                       d_lo, d_hi, inside, n_frames, d_frame_counts, false, 0, nullptr, nullptr, nullptr, nullptr, stream, verify);
}

int fa_find_count_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                          const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return find_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, n_sel, d_sel_streams, max_temp_bytes, d_lo, d_hi, inside,
                       n_frames, d_frame_counts, false, 0, nullptr, nullptr, nullptr, nullptr, stream, verify);
}

int fa_find_fill_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, const int64_t* d_lo,
                            const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                            const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify) {
    return find_device(1, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, 0, d_lo, d_hi,
                       inside, n_frames, nullptr, true, n_hit_tasks, d_hit_tasks, d_frame_offsets, d_pos, d_val, stream, verify);
}

int fa_find_fill_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                            const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                            const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify) {
    return find_device(2, nullptr, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first, last, n_sel, d_sel_streams, max_temp_bytes,
                       d_lo, d_hi, inside, n_frames, nullptr, true, n_hit_tasks, d_hit_tasks, d_frame_offsets, d_pos, d_val, stream, verify);
}

int fa_find_fill_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                         const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                         const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify) {
    DecodeIndex* ix = reinterpret_cast<DecodeIndex*>(index);
    if (!ix) return FA_ERROR_DECODE_INIT;
    return find_device(ix->nch, ix, nullptr, 0, nullptr, nullptr, 0, 0, first, last, n_sel, d_sel_streams, max_temp_bytes, d_lo, d_hi, inside,
                       n_frames, nullptr, true, n_hit_tasks, d_hit_tasks, d_frame_offsets, d_pos, d_val, stream, verify);
}

// ---- damage map and salvage decode (scrub_kernels.hpp) ----
// What the status pass leaves behind for a decode through it: the (realigned) blob and the tolerant tables.
struct ScrubTables {
    const unsigned char* bytes = nullptr;
    StreamMeta* meta = nullptr;
    int64_t* ftab = nullptr;
    int* err = nullptr;  // 64 ints, cleared: the decode's error block
    int64_t nf = 0;
};

// The status pass over the whole store, queued on `st` (not waited for).  Non-zero for bad arguments and HIP failures only.
static int scrub_run(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                     int64_t stream_size, int channels, int64_t block_size, unsigned char* d_status, hipStream_t st, ScrubTables* tb) {
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (channels != 1 && channels != 2) return FA_ERROR_CONVERT_TYPE;
    if (block_size < 1 || block_size > 65535) return FA_ERROR_DECODE_INIT;
    if (n_bytes < 0 || !d_starts || !d_nbytes || !d_status || (n_bytes > 0 && !d_bytes)) return FA_ERROR_DECODE_INIT;
    const int32_t B = (int32_t)block_size;
    const int64_t nf = (stream_size + B - 1) / B;
    if (nf > (int64_t)0x7fffffff * 4 / n_stream) return FA_ERROR_DECODE_SAMPLE_RANGE;  // one wavefront per frame, four per workgroup
    const int64_t nt = n_stream * nf;
    // 16-byte loads of the decoders are issued relative to the blob base: realign as they do
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) {
        void* al = nullptr;
        int rc0 = get_scratch(17, (size_t)n_bytes + 256, &al);
        if (rc0) return rc0;
        FA_HIP_TRY(hipMemcpyAsync(al, d_bytes, (size_t)n_bytes, hipMemcpyDeviceToDevice, st));
        d_bytes = reinterpret_cast<const unsigned char*>(al);
    }
    const size_t meta_bytes = align_up((size_t)n_stream * sizeof(StreamMeta), 256);
    const size_t flag_bytes = align_up((size_t)n_stream, 256);
    void *p = nullptr, *pt = nullptr;
    int rc = get_scratch(18, meta_bytes + flag_bytes + 256, &p);
    if (rc) return rc;
    if ((rc = get_scratch(19, (size_t)nt * 8 + 256, &pt))) return rc;
    const uint16_t* tab = nullptr;
    if ((rc = get_crc_tab_fused(&tab))) return rc;
    StreamMeta* d_meta = reinterpret_cast<StreamMeta*>(p);
    uint8_t* d_located = reinterpret_cast<uint8_t*>(p) + meta_bytes;
    int* d_err = reinterpret_cast<int*>(reinterpret_cast<char*>(p) + meta_bytes + flag_bytes);
    int64_t* d_ftab = reinterpret_cast<int64_t*>(pt);
    FA_HIP_TRY(hipMemsetAsync(d_err, 0, 256, st));
    hipLaunchKernelGGL(scrub_streams_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, d_bytes, d_starts, d_nbytes, n_stream, nf,
                       n_bytes, B, (int32_t)channels, d_meta, d_located);
    hipLaunchKernelGGL(scrub_table_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, d_bytes, d_meta, d_located, n_stream, nf, B, d_ftab);
    hipLaunchKernelGGL(frame_status_kernel, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, st, d_bytes, n_bytes, d_meta, d_ftab, n_stream, nf, B,
                       stream_size, (int32_t)channels, tab, d_status);
    FA_HIP_TRY(hipGetLastError());
    if (tb) { tb->bytes = d_bytes; tb->meta = d_meta; tb->ftab = d_ftab; tb->err = d_err; tb->nf = nf; }
    return FA_ERROR_NONE;
}

int fa_frame_status_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                           int64_t stream_size, int channels, int64_t block_size, unsigned char* d_status, void* stream) {
    FA_API_LOCK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int rc = scrub_run(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, channels, block_size, d_status, st, nullptr);
    if (rc) return rc;
    FA_HIP_TRY(hipStreamSynchronize(st));  // (the tables are cached scratch: the next call may be on another stream)
    return FA_ERROR_NONE;
}

int fa_fill_ranges_device(void* d_out, int elem_bytes, int64_t n_ranges, const int64_t* d_off, const int64_t* d_count, const void* fill_value,
                          void* stream) {
    FA_API_LOCK;
    if (elem_bytes != 4 && elem_bytes != 8) return FA_ERROR_CONVERT_TYPE;
    if (n_ranges < 0 || !fill_value) return FA_ERROR_DECODE_SAMPLE_RANGE;
    if (n_ranges == 0) return FA_ERROR_NONE;
    if (!d_out || !d_off || !d_count) return FA_ERROR_DECODE_INIT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (elem_bytes == 4) launch_fill<int32_t>(d_out, n_ranges, d_off, d_count, fill_value, st);
    else launch_fill<int64_t>(d_out, n_ranges, d_off, d_count, fill_value, st);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

// Decode through errors: the status pass, then every frame of status 0 that touches the range through K7 / K7L and the
// fill value over the samples of every other one.  Exactly one of out_int / out_float is set.
static int salvage_run(int nch, const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first_sample, int64_t last_sample, void* out_int, void* out_float, const void* d_offsets,
                       const void* d_gains, int64_t block_size, const void* fill_value, unsigned char* d_status, void* stream) {
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    int rc = check_output_args(out_int, out_float, d_offsets, d_gains);
    if (rc) return rc;
    if (!fill_value) return FA_ERROR_CONVERT_TYPE;
    int64_t first_decode, n_decode;
    if ((rc = validate_range(stream_size, first_sample, last_sample, &first_decode, &n_decode))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScrubTables tb;
    if ((rc = scrub_run(d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, nch, block_size, d_status, st, &tb))) return rc;
    const int64_t B = block_size, nf = tb.nf;
    std::vector<unsigned char> h_status((size_t)(n_stream * nf));
    FA_HIP_TRY(hipMemcpyAsync(h_status.data(), d_status, h_status.size(), hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    const int64_t f0 = first_decode / B, f1 = (first_decode + n_decode - 1) / B, last_decode = first_decode + n_decode;
    // runs of frames inside [f0, f1]: decodable ones become slices, the others fill ranges, both clipped to the range
    std::vector<int64_t> sl_stream, sl_first, sl_count, sl_out, fill_off, fill_count;
    int64_t n_tasks = 0;
    for (int64_t s = 0; s < n_stream; ++s) {
        const unsigned char* row = h_status.data() + s * nf;
        for (int64_t f = f0; f <= f1;) {
            const bool good = (row[f] == 0);
            int64_t g = f + 1;
            while (g <= f1 && (row[g] == 0) == good) ++g;
            const int64_t lo = std::max(f * B, first_decode), hi = std::min(g * B, last_decode);
            if (good) {
                sl_stream.push_back(s); sl_first.push_back(lo); sl_count.push_back(hi - lo); sl_out.push_back(s * n_decode + (lo - first_decode));
                n_tasks += g - f;
            } else {
                fill_off.push_back(s * n_decode + (lo - first_decode)); fill_count.push_back(hi - lo);
            }
            f = g;
        }
    }
    // the decode reads the tolerant tables as an index: it looks at neither d_starts / d_nbytes nor the strict K6
    DecodeIndex ix;
    ix.bytes = tb.bytes; ix.n_bytes = n_bytes; ix.n_stream = n_stream; ix.stream_size = stream_size; ix.nf = nf;
    ix.B = (int32_t)B; ix.nch = nch; ix.meta = tb.meta; ix.ftab = tb.ftab; ix.err = tb.err;
    (void)hipGetDevice(&ix.device);
    DecodeRequest r;  // (the frames were just checked: verify = 0)
    r.idx = &ix; r.nch = nch; r.st = st; r.verify = 0;
    r.output(out_int, out_float, d_offsets, d_gains);
    if (fill_off.empty()) {  // every frame of the range is intact: the ordinary grid-mode decode
        r.first = first_decode; r.n_decode = n_decode;
        return decode_device_impl(r);
    }
    {
        const int64_t nr = (int64_t)fill_off.size();
        void* pr = nullptr;
        if ((rc = get_scratch(21, (size_t)nr * 16 + 256, &pr))) return rc;
        int64_t* d_off = reinterpret_cast<int64_t*>(pr);
        int64_t* d_cnt = d_off + nr;
        FA_HIP_TRY(hipMemcpyAsync(d_off, fill_off.data(), (size_t)nr * 8, hipMemcpyHostToDevice, st));
        FA_HIP_TRY(hipMemcpyAsync(d_cnt, fill_count.data(), (size_t)nr * 8, hipMemcpyHostToDevice, st));
        void* const out = out_int ? out_int : out_float;
        if (nch == 1) { if (out_float) launch_fill<float>(out, nr, d_off, d_cnt, fill_value, st); else launch_fill<int32_t>(out, nr, d_off, d_cnt, fill_value, st); }
        else { if (out_float) launch_fill<double>(out, nr, d_off, d_cnt, fill_value, st); else launch_fill<int64_t>(out, nr, d_off, d_cnt, fill_value, st); }
        FA_HIP_TRY(hipGetLastError());
    }
    if (!sl_stream.empty()) {
        void* pk = nullptr;
        const size_t task_bytes = task_table_bytes(n_tasks);
        if ((rc = get_scratch(20, task_bytes + 4096, &pk))) return rc;
        ix.tasks = pk; ix.tasks_bytes = task_bytes + 4096;  // (large enough: the decode never grows, and never owns, this table)
        rc = decode_device_impl(r.slices((int64_t)sl_stream.size(), sl_stream.data(), sl_first.data(), sl_count.data(), sl_out.data()));
    }
    FA_HIP_TRY(hipStreamSynchronize(st));  // (the fill ranges' host vectors go out of scope)
    return rc;
}

int fa_decode_salvage_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                                 int64_t stream_size, int64_t first_sample, int64_t last_sample, int32_t* d_out_i32, float* d_out_f32,
                                 const float* d_offsets, const float* d_gains, int64_t block_size, const void* fill_value, unsigned char* d_status,
                                 void* stream) {
    return salvage_run(1, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first_sample, last_sample, d_out_i32, d_out_f32, d_offsets,
                       d_gains, block_size, fill_value, d_status, stream);
}

int fa_decode_salvage_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                                 int64_t stream_size, int64_t first_sample, int64_t last_sample, int64_t* d_out_i64, double* d_out_f64,
                                 const double* d_offsets, const double* d_gains, int64_t block_size, const void* fill_value, unsigned char* d_status,
                                 void* stream) {
    return salvage_run(2, d_bytes, n_bytes, d_starts, d_nbytes, n_stream, stream_size, first_sample, last_sample, d_out_i64, d_out_f64, d_offsets,
                       d_gains, block_size, fill_value, d_status, stream);
}

// ---- reindex (reindex_kernels.hpp) ----
int64_t fa_reindex_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t block_size) {
    if (n_old_bytes < 0 || n_stream < 0 || stream_size <= 0 || block_size < 1 || block_size > 65535) return -1;
    const int64_t nf = (stream_size + block_size - 1) / block_size;
    if (nf > kReindexMaxFrames) return -1;
    if (n_stream > 0 && stream_header_bytes(nf) > (INT64_MAX - n_old_bytes) / n_stream) return -1;
    return n_old_bytes + n_stream * stream_header_bytes(nf);  // (an upper bound: the bodies are part of the old bytes)
}

// K6's tables of the caller's store (built as a decode index is, freed on return), the check, the sizes and starts (one
// wait: the error word and the total), then the copy.  Nothing is written to d_bytes unless every check passed.
// Every launch and copy is on the caller's stream; the tables, like a decode index's, come from hipMalloc and go back
// with hipFree, and both wait for the whole device -- a one-time migration pays that, a call per read would not.
int fa_reindex_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                      int64_t n_stream, int64_t stream_size, int n_channels, unsigned char* d_bytes, int64_t capacity_bytes,
                      int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    FA_API_LOCK;
    if (!h_total_bytes) return FA_ERROR_ALLOC;
    *h_total_bytes = 0;
    if (n_stream < 0) return FA_ERROR_ZERO_NSTREAM;
    if (n_stream == 0) return FA_ERROR_NONE;  // an empty store: nothing to launch
    if (stream_size <= 0) return FA_ERROR_DECODE_STREAMSIZE;
    if (n_channels != 1 && n_channels != 2) return FA_ERROR_CONVERT_TYPE;
    if (n_old_bytes <= 0 || !d_old || !d_old_starts || !d_old_nbytes || !d_starts || !d_nbytes) return FA_ERROR_DECODE_INIT;
    if (!d_bytes || capacity_bytes <= 0) return FA_ERROR_ALLOC;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DecodeIndex ix;
    struct Tables {  // (hipFree waits for the device: the kernels that read the tables are done)
        DecodeIndex* ix;
        ~Tables() {
            if (ix->meta) (void)hipFree(ix->meta);
            if (ix->ftab) (void)hipFree(ix->ftab);
        }
    } tables{&ix};
    // (a store that is not 16-byte aligned is read from K6's realigned copy in the decoders' slot: calls are serialised
    // by api_mu and each writes the slot before it reads it, so one store-sized buffer serves both)
    int rc = build_decode_tables(d_old, n_old_bytes, d_old_starts, d_old_nbytes, n_stream, stream_size, n_channels, st, true, &ix);
    if (rc) return rc;  // (K6's own errors: a bad header, variable or mixed block sizes, a walk that runs off its stream)
    d_old = ix.bytes;
    if (ix.nf > kReindexMaxFrames) return FA_ERROR_DECODE_INIT;
    const int64_t nt = n_stream * ix.nf;
    if (nt >= (1LL << 31) * 256) return FA_ERROR_DECODE_SAMPLE_RANGE;
    void* ps = nullptr;
    if ((rc = get_scratch(22, 256, &ps))) return rc;
    ReindexArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = d_old; a.src_bytes = n_old_bytes; a.src_starts = d_old_starts; a.meta = ix.meta; a.ftab = ix.ftab;
    a.starts = d_starts; a.nbytes = d_nbytes; a.out = d_bytes;
    a.err = reinterpret_cast<int*>(ps);
    a.n_stream = n_stream; a.nf = ix.nf; a.stream_size = stream_size; a.B = ix.B;
    int64_t* d_total = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ps) + 8);
    FA_HIP_TRY(hipMemsetAsync(ps, 0, 16, st));
    hipLaunchKernelGGL(reindex_check_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(reindex_size_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(1024), 0, st, d_nbytes, n_stream, d_starts, d_total);
    struct { int32_t err, pad; int64_t total; } back = {0, 0, 0};
    FA_HIP_TRY(hipMemcpyAsync(&back, ps, sizeof back, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (back.err & kReindexBadHeader) return FA_ERROR_DECODE_INIT;
    if (back.err & kReindexBadTable) return FA_ERROR_DECODE_SEEK;
    if (back.err) return FA_ERROR_DECODE_STREAMSIZE;  // (the last frame is not frame nf - 1 of the stream_size given)
    if (back.total > capacity_bytes) return FA_ERROR_ALLOC;
    // workgroups per stream: ~64 KB of the result each (at most 1024, and a grid of fewer than 2^23 workgroups)
    int64_t parts = std::max<int64_t>(1, std::min<int64_t>(1024, back.total / n_stream / 65536));
    while (parts > 1 && n_stream * parts >= (1LL << 23)) parts >>= 1;
    if (n_stream * parts >= (1LL << 23)) return FA_ERROR_DECODE_SAMPLE_RANGE;  // (parts == 1: more streams than a grid takes)
    a.parts = (int32_t)parts;
    hipLaunchKernelGGL(reindex_kernel, dim3((unsigned)(n_stream * parts)), dim3(256), 0, st, a);
    FA_HIP_TRY(hipGetLastError());
    FA_HIP_TRY(hipStreamSynchronize(st));  // (the tables are freed on return, the scratch is the next call's)
    *h_total_bytes = back.total;
    return FA_ERROR_NONE;
}

// ---- window (window_kernels.hpp, K14): the kept frames renumbered downwards, a cut inside a frame re-encoded ----------
// Workspace layout (256-byte aligned regions): the picked streams' starts | nbytes, the output row of every stream, the
// error word and total; with a tail (last inside an old frame) the decoded (m, r) image, the encode's blob (its capacity),
// its starts | nbytes and the encode's own workspace.
struct WindowPlan {
    int64_t B, nf_old, f0, nk, nchk, nf_new, r, enc_cap, enc_ws;
    bool tail, whole;
    size_t off_sub, off_slot, off_small, off_img, off_blob, off_idx, off_ws, total;
};
static int make_window_plan(int nch, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t last, uint32_t level,
                            WindowPlan* pl) {
    if (nch != 1 && nch != 2) return FA_ERROR_CONVERT_TYPE;
    FramePlan old;
    const int rc = make_frame_plan(n_stream, stream_size, level, nch, &old);
    if (rc && rc != FA_ERROR_ENCODE_PROCESS) return rc;  // (the limits were the old store's own encode's to refuse)
    if (m < 0 || m > n_stream) return FA_ERROR_ZERO_NSTREAM;
    if (first < 0 || last > stream_size || last <= first) return FA_ERROR_DECODE_SAMPLE_RANGE;
    pl->B = old.B;
    pl->nf_old = old.nf;
    if (first % pl->B) return FA_ERROR_DECODE_SAMPLE_RANGE;  // every frame boundary moves: nothing to copy, the caller encodes
    const int64_t n = last - first;
    pl->f0 = first / pl->B;
    pl->whole = (first == 0 && last == stream_size);
    if (last == stream_size) {  // the old last frame, short or not, is one more kept frame
        pl->nk = pl->nf_old - pl->f0;
        pl->r = 0;
    } else {
        pl->nk = n / pl->B;
        pl->r = n % pl->B;
    }
    pl->tail = pl->r != 0;
    pl->nf_new = pl->nk + (pl->tail ? 1 : 0);
    pl->nchk = pl->whole ? 1 : pl->nf_new;
    pl->enc_cap = pl->enc_ws = 0;
    if (pl->tail && m > 0) {
        FramePlan enc;  // the encode of the (m, r) image: one short frame per stream
        if (make_frame_plan(m, pl->r, level, nch, &enc) != FA_ERROR_NONE) return FA_ERROR_ENCODE_INIT;
        pl->enc_cap = enc.capacity;
        pl->enc_ws = single_pass_workspace_for(m, pl->r, level, nch);
    }
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    pl->off_sub = o; o += up((size_t)m * 16);
    pl->off_slot = o; o += up((size_t)n_stream * 4);
    pl->off_small = o; o += 256;
    pl->off_img = o; o += pl->tail ? up((size_t)m * (size_t)pl->r * 4 * (size_t)nch) : 0;
    pl->off_blob = o; o += pl->tail ? up((size_t)pl->enc_cap + 64) : 0;
    pl->off_idx = o; o += pl->tail ? up((size_t)m * 16) : 0;
    pl->off_ws = o; o += up((size_t)pl->enc_ws);
    pl->total = o;
    return FA_ERROR_NONE;
}

int64_t fa_window_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t last, int channels, uint32_t level) {
    WindowPlan pl;
    return make_window_plan(channels, n_stream, stream_size, m, first, last, level, &pl) ? -1 : (int64_t)pl.total;
}
// a picked stream's header and kept frames only shrink; what can grow is the re-encoded tail frame, bounded by its encode
int64_t fa_window_capacity_bytes(int64_t n_picked_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t last, int channels,
                                 uint32_t level) {
    WindowPlan pl;
    if (n_picked_bytes < 0 || make_window_plan(channels, n_stream, stream_size, m, first, last, level, &pl)) return -1;
    return n_picked_bytes + pl.enc_cap + 6 * m + 64;
}

int fa_window_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes, int64_t n_stream,
                     int64_t stream_size, const int64_t* d_stream_index, int64_t m, int64_t first, int64_t last, int channels, uint32_t level,
                     void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                     int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    FA_API_LOCK;
    if (!h_total_bytes) return FA_ERROR_ALLOC;
    *h_total_bytes = 0;
    if (!d_stream_index && m != n_stream && m != 0) return FA_ERROR_ZERO_NSTREAM;
    WindowPlan pl;
    int rc = make_window_plan(channels, n_stream, stream_size, m, first, last, level, &pl);
    if (rc) return rc;
    if (m == 0) return FA_ERROR_NONE;  // an empty store: nothing to launch
    if (n_old_bytes <= 0 || !d_old || !d_old_starts || !d_old_nbytes || !d_starts || !d_nbytes) return FA_ERROR_DECODE_INIT;
    if (!d_workspace || workspace_bytes < (int64_t)pl.total) return FA_ERROR_ALLOC;
    if (!d_bytes || capacity_bytes <= 0) return FA_ERROR_ALLOC;
    // (the copy reads its sources in aligned 16-byte blocks)
    if ((reinterpret_cast<uintptr_t>(d_old) & 15) || (reinterpret_cast<uintptr_t>(d_workspace) & 15)) return FA_ERROR_ENCODE_INIT;
    const int nch = channels;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    WindowArgs a;
    std::memset(&a, 0, sizeof a);
    a.old = d_old; a.old_bytes = n_old_bytes; a.old_starts = d_old_starts; a.old_nbytes = d_old_nbytes;
    a.sidx = d_stream_index;
    a.slot = reinterpret_cast<int32_t*>(ws + pl.off_slot);
    a.sub_starts = reinterpret_cast<int64_t*>(ws + pl.off_sub);
    a.sub_nbytes = a.sub_starts + m;
    a.starts = d_starts; a.nbytes = d_nbytes; a.out = d_bytes;
    a.err = reinterpret_cast<int*>(ws + pl.off_small);
    a.n_stream = n_stream; a.m = m; a.size_old = stream_size; a.size_new = last - first;
    a.f0 = pl.f0; a.nk = pl.nk; a.nchk = pl.nchk; a.nf_old = pl.nf_old; a.nf_new = pl.nf_new;
    a.B = (int32_t)pl.B; a.nch = nch; a.tail = pl.tail ? 1 : 0; a.whole = pl.whole ? 1 : 0;
    // 0. the stream index, the layout of every picked stream, and every seek offset the copy or the tail decode follows
    const int64_t nt = m * pl.nchk;
    if (nt >= (1LL << 31) * 256) return FA_ERROR_DECODE_SAMPLE_RANGE;
    FA_HIP_TRY(hipMemsetAsync(ws + pl.off_small, 0, 16, st));
    FA_HIP_TRY(hipMemsetAsync(a.sub_starts, 0, (size_t)m * 16, st));
    if (d_stream_index) {
        FA_HIP_TRY(hipMemsetAsync(a.slot, 0xFF, (size_t)n_stream * 4, st));
    }
    hipLaunchKernelGGL(window_check_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, a);
    {
        int h_err = 0;
        FA_HIP_TRY(hipMemcpyAsync(&h_err, a.err, sizeof h_err, hipMemcpyDeviceToHost, st));
        FA_HIP_TRY(hipStreamSynchronize(st));
        FA_HIP_TRY(hipGetLastError());
        if (h_err & kWindowBadIndex) return FA_ERROR_ZERO_NSTREAM;
        if (h_err & kWindowBadLayout) return FA_ERROR_DECODE_INIT;
        if (h_err) return FA_ERROR_DECODE_SEEK;
    }
    // 1. the tail: old frame f0 + nk decoded up to the cut, encoded again as one short frame per stream, numbered 0
    if (pl.tail) {
        char* img = ws + pl.off_img;
        const int64_t lo = (pl.f0 + pl.nk) * pl.B;
        rc = decode_span(nch, d_old, n_old_bytes, a.sub_starts, a.sub_nbytes, m, stream_size, lo, last, img, stream);
        if (rc) return rc;
        unsigned char* blob = reinterpret_cast<unsigned char*>(ws + pl.off_blob);
        int64_t* e_idx = reinterpret_cast<int64_t*>(ws + pl.off_idx);
        int64_t enc_total = 0;
        rc = encode_image(nch, img, m, pl.r, level, ws + pl.off_ws, pl.enc_ws, blob, pl.enc_cap, e_idx, &enc_total, stream);
        if (rc) return rc;
        a.enc = blob; a.enc_bytes = enc_total; a.enc_starts = e_idx; a.enc_nbytes = e_idx + m;
    }
    // 2. sizes, starts (one wait: the error word and the total), then the copy
    int64_t* d_total = reinterpret_cast<int64_t*>(ws + pl.off_small + 8);
    FA_HIP_TRY(hipMemsetAsync(ws + pl.off_small, 0, 16, st));
    hipLaunchKernelGGL(window_size_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(1024), 0, st, d_nbytes, m, d_starts, d_total);
    struct { int32_t err, pad; int64_t total; } back = {0, 0, 0};
    FA_HIP_TRY(hipMemcpyAsync(&back, a.err, sizeof back, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (back.err) return FA_ERROR_DECODE_INIT;  // (the tail encode's index)
    if (back.total > capacity_bytes) return FA_ERROR_ALLOC;
    // workgroups per stream: ~64 KB of the result each (at most 1024, and a grid of fewer than 2^23 workgroups)
    int64_t parts = std::max<int64_t>(1, std::min<int64_t>(1024, back.total / m / 65536));
    while (parts > 1 && m * parts >= (1LL << 23)) parts >>= 1;
    if (m * parts >= (1LL << 23)) return FA_ERROR_ALLOC;
    a.parts = (int32_t)parts;
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)(m * parts)), dim3(256), 0, st, a);
    FA_HIP_TRY(hipGetLastError());
    *h_total_bytes = back.total;
    return FA_ERROR_NONE;
}

// ---- join (join_kernels.hpp, K15): the parts' frames behind one another, renumbered upwards ------------------------------
// Workspace layout (256-byte aligned regions): the part descriptors, D_p(s) for every part and stream, the error word and
// total.
struct JoinPlan {
    int64_t B, nf_new, size_new, growth_sum;
    std::vector<int64_t> nf, base, growth;
    bool whole;
    size_t off_parts, off_D, off_small, total;
};
static int make_join_plan(int nch, int64_t n_parts, int64_t n_stream, const int64_t* sizes, uint32_t level, JoinPlan* pl) {
    if (nch != 1 && nch != 2) return FA_ERROR_CONVERT_TYPE;
    if (level > 8) return FA_ERROR_INVALID_LEVEL;
    if (n_parts <= 0 || n_stream < 0) return FA_ERROR_ZERO_NSTREAM;
    if (n_parts > kJoinMaxParts) return FA_ERROR_ENCODE_PROCESS;  // (an implementation limit: join in groups)
    if (!sizes) return FA_ERROR_DECODE_INIT;
    pl->B = level_params(level).blocksize;
    pl->nf.resize((size_t)n_parts); pl->base.resize((size_t)n_parts); pl->growth.resize((size_t)n_parts);
    int64_t total = 0;
    for (int64_t p = 0; p < n_parts; ++p) {
        if (sizes[p] <= 0) return FA_ERROR_ZERO_STREAMSIZE;
        if (sizes[p] >= (1LL << 36) || (total += sizes[p]) >= (1LL << 36)) return FA_ERROR_DECODE_SAMPLE_RANGE;  // STREAMINFO holds 36 bits
    }
    total = 0;
    pl->growth_sum = 0;
    for (int64_t p = 0; p < n_parts; ++p) {
        // every frame boundary behind an unaligned part moves: nothing to copy there, the caller decodes and encodes
        if (total % pl->B) return FA_ERROR_DECODE_SAMPLE_RANGE;
        pl->nf[(size_t)p] = (sizes[p] + pl->B - 1) / pl->B;
        pl->base[(size_t)p] = total / pl->B;
        pl->growth[(size_t)p] = append_growth(pl->base[(size_t)p], pl->nf[(size_t)p]);
        pl->growth_sum += pl->growth[(size_t)p];
        total += sizes[p];
    }
    pl->size_new = total;
    pl->nf_new = pl->base[(size_t)n_parts - 1] + pl->nf[(size_t)n_parts - 1];
    if (18 * pl->nf_new >= (1 << 24)) return FA_ERROR_ENCODE_PROCESS;  // SEEKTABLE block length is 24 bit
    pl->whole = n_parts == 1;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    pl->off_parts = o; o += up((size_t)n_parts * sizeof(JoinPart));
    pl->off_D = o; o += up((size_t)n_parts * (size_t)n_stream * 8);
    pl->off_small = o; o += 256;
    pl->total = o;
    return FA_ERROR_NONE;
}

int64_t fa_join_workspace_bytes(int64_t n_parts, int64_t n_stream, const int64_t* stream_sizes, int channels, uint32_t level) {
    JoinPlan pl;
    return make_join_plan(channels, n_parts, n_stream, stream_sizes, level, &pl) ? -1 : (int64_t)pl.total;
}
// new size of stream s = 46 + sum_p (nbytes_p(s) - 46 + growth_p): the seek points only move
int64_t fa_join_capacity_bytes(int64_t n_parts, const int64_t* n_old_bytes, int64_t n_stream, const int64_t* stream_sizes, int channels,
                               uint32_t level) {
    JoinPlan pl;
    if (make_join_plan(channels, n_parts, n_stream, stream_sizes, level, &pl) || !n_old_bytes) return -1;
    int64_t cap = n_stream * (46 + pl.growth_sum);
    for (int64_t p = 0; p < n_parts; ++p) {
        if (n_old_bytes[p] < 0 || n_old_bytes[p] > INT64_MAX - cap) return -1;
        cap += n_old_bytes[p];
    }
    return cap;
}

int fa_join_device(int64_t n_parts, const unsigned char* const* d_old, const int64_t* n_old_bytes, const int64_t* const* d_old_starts,
                   const int64_t* const* d_old_nbytes, const int64_t* stream_sizes, int64_t n_stream, int channels, uint32_t level,
                   void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                   int64_t* d_nbytes, int64_t* h_total_bytes, void* stream) {
    FA_API_LOCK;
    if (!h_total_bytes) return FA_ERROR_ALLOC;
    *h_total_bytes = 0;
    JoinPlan pl;
    int rc = make_join_plan(channels, n_parts, n_stream, stream_sizes, level, &pl);
    if (rc) return rc;
    if (n_stream == 0) return FA_ERROR_NONE;  // an empty store: nothing to launch
    if (!d_old || !n_old_bytes || !d_old_starts || !d_old_nbytes || !d_starts || !d_nbytes) return FA_ERROR_DECODE_INIT;
    for (int64_t p = 0; p < n_parts; ++p)
        if (n_old_bytes[p] <= 0 || !d_old[p] || !d_old_starts[p] || !d_old_nbytes[p]) return FA_ERROR_DECODE_INIT;
    if (!d_workspace || workspace_bytes < (int64_t)pl.total) return FA_ERROR_ALLOC;
    if (!d_bytes || capacity_bytes <= 0) return FA_ERROR_ALLOC;
    // (the copy reads its sources in aligned 16-byte blocks)
    if (reinterpret_cast<uintptr_t>(d_workspace) & 15) return FA_ERROR_ENCODE_INIT;
    for (int64_t p = 0; p < n_parts; ++p)
        if (reinterpret_cast<uintptr_t>(d_old[p]) & 15) return FA_ERROR_ENCODE_INIT;
    const int64_t nchk = pl.whole ? 1 : pl.nf_new;
    const int64_t nt = n_stream * nchk;
    if (nt >= (1LL << 31) * 256) return FA_ERROR_DECODE_SAMPLE_RANGE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    std::vector<JoinPart> h_parts((size_t)n_parts);
    for (int64_t p = 0; p < n_parts; ++p) {
        JoinPart& q = h_parts[(size_t)p];
        q.old = d_old[p]; q.old_bytes = n_old_bytes[p]; q.old_starts = d_old_starts[p]; q.old_nbytes = d_old_nbytes[p];
        q.size = stream_sizes[p]; q.nf = pl.nf[(size_t)p]; q.base = pl.base[(size_t)p]; q.growth = pl.growth[(size_t)p];
    }
    JoinArgs a;
    std::memset(&a, 0, sizeof a);
    a.part = reinterpret_cast<const JoinPart*>(ws + pl.off_parts);
    a.D = reinterpret_cast<int64_t*>(ws + pl.off_D);
    a.starts = d_starts; a.nbytes = d_nbytes; a.out = d_bytes;
    a.err = reinterpret_cast<int*>(ws + pl.off_small);
    a.P = n_parts; a.n_stream = n_stream; a.size_new = pl.size_new; a.nf_new = pl.nf_new; a.nchk = nchk;
    a.B = (int32_t)pl.B; a.nch = channels; a.whole = pl.whole ? 1 : 0;
    // 0. the layout of every stream of every part and every seek offset the copy follows; 1. sizes and starts (one wait:
    // the error word and the total, which also keeps the host's descriptors alive until they are uploaded)
    int64_t* d_total = reinterpret_cast<int64_t*>(ws + pl.off_small + 8);
    FA_HIP_TRY(hipMemsetAsync(ws + pl.off_small, 0, 16, st));
    FA_HIP_TRY(hipMemcpyAsync(ws + pl.off_parts, h_parts.data(), (size_t)n_parts * sizeof(JoinPart), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(join_check_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(join_size_kernel, dim3((unsigned)((n_stream + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(1024), 0, st, d_nbytes, n_stream, d_starts, d_total);
    struct { int32_t err, pad; int64_t total; } back = {0, 0, 0};
    FA_HIP_TRY(hipMemcpyAsync(&back, a.err, sizeof back, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    if (back.err & kJoinBadLayout) return FA_ERROR_DECODE_INIT;
    if (back.err) return FA_ERROR_DECODE_SEEK;
    if (back.total <= 0 || back.total > capacity_bytes) return FA_ERROR_ALLOC;
    // 2. the copy.  Workgroups per stream: ~64 KB of the result each (at most 1024, and a grid of fewer than 2^23 workgroups)
    int64_t parts = std::max<int64_t>(1, std::min<int64_t>(1024, back.total / n_stream / 65536));
    while (parts > 1 && n_stream * parts >= (1LL << 23)) parts >>= 1;
    if (n_stream * parts >= (1LL << 23)) return FA_ERROR_ALLOC;
    a.parts = (int32_t)parts;
    hipLaunchKernelGGL(join_kernel, dim3((unsigned)(n_stream * parts)), dim3(256), 0, st, a);
    FA_HIP_TRY(hipGetLastError());
    *h_total_bytes = back.total;
    return FA_ERROR_NONE;
}

int fa_float32_to_int32_device(const float* d_input, int64_t n_stream, int64_t stream_size, const float* d_quanta,
                               int32_t* d_output, float* d_offsets, float* d_gains, void* stream) {
    if (n_stream > INT32_MAX) return FA_ERROR_CONVERT_TYPE;  // one workgroup per stream: the grid's bound (before anything is touched)
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* p = nullptr;
    int rc = get_scratch(4, 256, &p);
    if (rc) return rc;
    int* d_flags = reinterpret_cast<int*>(p);
    FA_HIP_TRY(hipMemsetAsync(d_flags, 0, 4, st));
    prof_begin(5, st);
    hipLaunchKernelGGL(float32_to_int32_kernel, dim3((unsigned)n_stream), dim3(1024), 0, st, d_input, stream_size, d_quanta,
                       d_output, d_offsets, d_gains, d_flags);
    prof_end(5, st);
    int h = 0;
    FA_HIP_TRY(hipMemcpyAsync(&h, d_flags, 4, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    return (h & 1) ? FA_ERROR_NAN_INPUT : FA_ERROR_NONE;
}

int fa_int32_to_float32_device(const int32_t* d_input, int64_t n_stream, int64_t stream_size, const float* d_offsets,
                               const float* d_gains, float* d_output, void* stream) {
    if (n_stream <= 0 || stream_size <= 0) return FA_ERROR_NONE;
    const int64_t cps = (stream_size - 1) / kDequantChunk + 1;
    if (n_stream > INT32_MAX / cps) return FA_ERROR_CONVERT_TYPE;  // one workgroup per chunk: the grid's bound (before anything is touched)
    FA_API_LOCK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(int32_to_float32_kernel, dim3((unsigned)(n_stream * cps)), dim3(256), 0, st, d_input, stream_size, cps,
                       d_offsets, d_gains, d_output);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

int fa_float64_to_int64_device(const double* d_input, int64_t n_stream, int64_t stream_size, const double* d_quanta,
                               int64_t* d_output, double* d_offsets, double* d_gains, void* stream) {
    if (n_stream > INT32_MAX) return FA_ERROR_CONVERT_TYPE;  // one workgroup per stream: the grid's bound (before anything is touched)
    FA_API_LOCK;
    if (n_stream <= 0) return FA_ERROR_ZERO_NSTREAM;
    if (stream_size <= 0) return FA_ERROR_ZERO_STREAMSIZE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* p = nullptr;
    int rc = get_scratch(4, 256, &p);
    if (rc) return rc;
    int* d_flags = reinterpret_cast<int*>(p);
    FA_HIP_TRY(hipMemsetAsync(d_flags, 0, 4, st));
    hipLaunchKernelGGL(float64_to_int64_kernel, dim3((unsigned)n_stream), dim3(1024), 0, st, d_input, stream_size, d_quanta,
                       d_output, d_offsets, d_gains, d_flags);
    int h = 0;
    FA_HIP_TRY(hipMemcpyAsync(&h, d_flags, 4, hipMemcpyDeviceToHost, st));
    FA_HIP_TRY(hipStreamSynchronize(st));
    FA_HIP_TRY(hipGetLastError());
    return (h & 1) ? FA_ERROR_NAN_INPUT : FA_ERROR_NONE;
}

int fa_int64_to_float64_device(const int64_t* d_input, int64_t n_stream, int64_t stream_size, const double* d_offsets,
                               const double* d_gains, double* d_output, void* stream) {
    if (n_stream <= 0 || stream_size <= 0) return FA_ERROR_NONE;
    const int64_t cps = (stream_size - 1) / kDequantChunk + 1;
    if (n_stream > INT32_MAX / cps) return FA_ERROR_CONVERT_TYPE;  // one workgroup per chunk: the grid's bound (before anything is touched)
    FA_API_LOCK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(int64_to_float64_kernel, dim3((unsigned)(n_stream * cps)), dim3(256), 0, st, d_input, stream_size, cps,
                       d_offsets, d_gains, d_output);
    FA_HIP_TRY(hipGetLastError());
    return FA_ERROR_NONE;
}

int fa_stream_std_f32_device(const float* d_in, int64_t n_stream, int64_t stream_size, int64_t chunk, float* d_out, void* stream) {
    return stream_std_impl<float>(d_in, n_stream, stream_size, chunk, d_out, stream);
}

int fa_stream_std_f64_device(const double* d_in, int64_t n_stream, int64_t stream_size, int64_t chunk, double* d_out, void* stream) {
    return stream_std_impl<double>(d_in, n_stream, stream_size, chunk, d_out, stream);
}

// ---------------------------------------------------------------------------------------------
// Host-pointer drop-ins (reference C ABI).  Data makes a PCIe round trip: the array is cut into chunks of
// ~256 MiB, a feeder thread uploads chunk c+1 on its own stream while this thread runs the kernels of chunk c and
// copies its result back (PCIe is full duplex), and the pages of freshly allocated host memory -- the malloc()'d blob
// of the encoder, the caller's output array of the decoder -- are populated by helper threads ahead of the copies
// (first-touch faults alone ran at 16 GB/s against the link's 56, tools/pcie_probe.py).  Device memory in use: two
// input chunks + one output chunk, whatever the array's size.
// ---------------------------------------------------------------------------------------------
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23  // Linux >= 5.14: fault pages in, writable, without touching their contents
#endif

// Populate [p, p + n) (the page-aligned inside of it) on a helper thread; join() before the memory is freed.  Contents
// are never written, so the helper may run beside DMA into the same range.  On kernels without MADV_POPULATE_WRITE the
// call fails and nothing happens (the copies then fault the pages in themselves, at 16 GB/s instead of the link's 56).
// Measured on the MI355X box (profiles/r03_host_abi.md): fresh anonymous memory populates at 19 GB/s (26 with
// transparent huge pages) whatever the number of threads -- that rate, not PCIe, bounds both host entry points -- and a
// populate call holds the address space's lock, which the runtime's pinning of the copy buffers and thread creation
// need too: one helper working in 128 KiB pieces lets the uploads through (4 helpers on 32 MiB pieces delayed the
// first upload by 40 ms).
static double host_now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static bool host_trace() {  // FLACARRAY_HIP_HOST_TRACE=1: per-chunk timeline of the host entry points on stderr (tools/host_trace.py)
    static const bool on = std::getenv("FLACARRAY_HIP_HOST_TRACE") != nullptr;
    return on;
}
#define FA_HTRACE(...) do { if (host_trace()) std::fprintf(stderr, __VA_ARGS__); } while (0)

struct PagePopulator {
    std::vector<std::thread> th;
    void start(void* p, size_t n, int nthreads, bool huge) {
        const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
        uintptr_t a = ((uintptr_t)p + pg - 1) & ~(pg - 1), b = ((uintptr_t)p + n) & ~(pg - 1);
        if (b <= a || n < (64u << 20)) return;
        if (huge) {
            const uintptr_t hp = 2u << 20;
            const uintptr_t ha = (a + hp - 1) & ~(hp - 1), hb = b & ~(hp - 1);
            if (hb > ha) (void)madvise((void*)ha, hb - ha, MADV_HUGEPAGE);
        }
        const uintptr_t piece = 128u << 10;
        auto next = std::make_shared<std::atomic<uintptr_t>>(a);
        const double t0 = host_now();
        for (int t = 0; t < nthreads; ++t) try {
            th.emplace_back([next, b, piece, t0, t] {
                for (;;) {
                    const uintptr_t lo = next->fetch_add(piece);
                    if (lo >= b) break;
                    const uintptr_t hi = lo + piece < b ? lo + piece : b;
                    if (madvise((void*)lo, hi - lo, MADV_POPULATE_WRITE) != 0) break;
                }
                FA_HTRACE("  populate thread %d done after %.2f ms\n", t, (host_now() - t0) * 1e3);
            });
        } catch (...) {  // no thread to be had: the copies fault the pages in themselves
            break;
        }
    }
    void join() {
        for (auto& t : th) t.join();
        th.clear();
    }
    ~PagePopulator() { join(); }
};

// Uploads: chunk c goes to slot c & 1 once chunk c - 2 has been consumed.  `upload(c, slot, stream)` issues the
// copies of one chunk; the thread waits for them and publishes the chunk.
struct Feeder {
    std::mutex mu;
    std::condition_variable cv;
    int64_t uploaded = 0, consumed = 0;  // chunks
    int err = FA_ERROR_NONE;
    bool stop = false;
    std::thread th;
    hipStream_t st = nullptr;
    int start(int dev, int64_t n_chunks, std::function<int(int64_t, int, hipStream_t)> upload, hipStream_t* cached) {
        if (!*cached && hipStreamCreateWithFlags(cached, hipStreamNonBlocking) != hipSuccess) return FA_ERROR_DEVICE;
        st = *cached;
        try {
        th = std::thread([this, dev, n_chunks, upload] {
            if (hipSetDevice(dev) != hipSuccess) { fail(FA_ERROR_DEVICE); return; }
            for (int64_t c = 0; c < n_chunks; ++c) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || consumed + 2 > c; });
                    if (stop) return;
                }
                const double t0 = host_now();
                int rc = upload(c, (int)(c & 1), st);
                if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = FA_ERROR_DEVICE;
                FA_HTRACE("  feeder: chunk %lld up in %.2f ms (started %.2f)\n", (long long)c, (host_now() - t0) * 1e3, t0 * 1e3);
                if (rc) { fail(rc); return; }
                { std::lock_guard<std::mutex> lk(mu); uploaded = c + 1; }
                cv.notify_all();
            }
        });
        } catch (...) {
            return FA_ERROR_ALLOC;  // (std::system_error: no thread)
        }
        return FA_ERROR_NONE;
    }
    void fail(int rc) {
        { std::lock_guard<std::mutex> lk(mu); err = rc; }
        cv.notify_all();
    }
    int wait_for(int64_t c) {  // chunk c is on the device (or the feeder failed)
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return err != FA_ERROR_NONE || uploaded > c; });
        return err;
    }
    void done_with(int64_t c) {
        { std::lock_guard<std::mutex> lk(mu); consumed = c + 1; }
        cv.notify_all();
    }
    void finish() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        st = nullptr;  // (the stream stays with the device state)
    }
    ~Feeder() { finish(); }
};

static int64_t host_chunk_streams(int64_t n_stream, size_t bytes_per_stream, int64_t max_by_grid, bool signing = false) {
    // ~256 MiB per chunk, at least 8 chunks for arrays that can afford them (the first upload and the last download are
    // not overlapped with anything), never more than the grid allows.  Signing: the MD5 of a chunk takes the time of ONE
    // stream's chain however many streams the chunk holds (md5_kernels.hpp), once per chunk -- so fewer, larger chunks.
    const size_t total = (size_t)n_stream * bytes_per_stream;
    size_t target = signing ? ((size_t)2048u << 20) : ((size_t)256u << 20);
    if (total / 8 < target) target = total / 8 > (32u << 20) ? total / 8 : (32u << 20);
    if (const char* e = std::getenv("FLACARRAY_HIP_HOST_CHUNK_BYTES")) {  // tests: many small chunks through the pipeline
        const long long v = std::atoll(e);
        if (v > 0) target = (size_t)v;
    }
    int64_t chunk = (int64_t)(target / (bytes_per_stream ? bytes_per_stream : 1));
    if (chunk < 1) chunk = 1;
    if (chunk > n_stream) chunk = n_stream;
    if (chunk > max_by_grid) chunk = max_by_grid;
    if (chunk > (1 << 20)) chunk = 1 << 20;
    return chunk;
}

// data: int32 (nch 1), int64 (nch 2) or float32 (f32: quantised on the device -- fused into the encoder where the
// geometry allows, utils.c:160-243; quanta may be null; offsets / gains [n_stream] are outputs)
// f64 (nch == 2): the input is float64 and is quantised to int64 on the device (float64_to_int64, utils.c:245-327) in
// front of the two-channel encoder; quanta64 may be null; offsets64 / gains64 [n_stream] are outputs.
static int encode_host(const void* data_v, int nch, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
                       int64_t* starts, unsigned char** bytes, bool f32 = false, const float* quanta = nullptr,
                       float* offsets = nullptr, float* gains = nullptr, bool f64 = false, const double* quanta64 = nullptr,
                       double* offsets64 = nullptr, double* gains64 = nullptr) {
    FA_API_LOCK;
    const double t_enter = host_now();
    if (level > 8) return FA_ERROR_INVALID_LEVEL;        // compress.c:144-146
    if (n_stream == 0) return FA_ERROR_ZERO_NSTREAM;     // compress.c:147-149
    if (stream_size == 0) return FA_ERROR_ZERO_STREAMSIZE;  // compress.c:150-152
    *n_bytes = 0;
    *bytes = nullptr;
    for (int64_t i = 0; i < n_stream; ++i) starts[i] = 0;
    if (n_stream < 0 || stream_size < 0) return FA_ERROR_ZERO_NSTREAM;
    if (fa_device_count() <= 0) return FA_ERROR_DEVICE;
    FramePlan one;  // one stream: frames per stream, and the worst case of a stream
    int rc = make_frame_plan(1, stream_size, level, nch, &one);
    if (rc) return rc;
    int dev = 0;
    FA_HIP_TRY(hipGetDevice(&dev));
    const unsigned char* data = reinterpret_cast<const unsigned char*>(data_v);
    const size_t stream_bytes = (size_t)stream_size * 4 * (size_t)nch;
    const bool verifying = g_encode_verify.load();
    const bool signing = g_encode_md5.load();
    // (verifying two-channel chunks also takes the decoder's planar image, as large again as the chunk's input)
    const int64_t chunk = host_chunk_streams(n_stream, stream_bytes * (verifying && nch == 2 ? 2 : 1), 0x7fffffffLL / one.nf, signing);
    const int64_t n_chunks = (n_stream + chunk - 1) / chunk;
    // (K3F's float geometries do not depend on the stream count: the last, smaller chunk takes the route of the others)
    FramePlan per_chunk;
    if ((rc = make_frame_plan(chunk, stream_size, level, nch, &per_chunk))) return rc;
    const bool fused_f32 = f32 && fused_geometry(per_chunk, true);

    // device buffers: two input slots, output, workspace, per-stream tables
    void *d_in2 = nullptr, *d_ws = nullptr, *d_aux = nullptr, *d_out = nullptr, *d_int = nullptr;
    const size_t in_b = (size_t)chunk * stream_bytes;
    const size_t in_slot = align_up(in_b, 256);
    if ((rc = get_scratch(0, 2 * in_slot + 256, &d_in2))) return rc;
    const int64_t wsb = single_pass_workspace_for(chunk, stream_size, level, nch);  // (the slot sequence's size when that is forced)
    if (wsb < 0) return FA_ERROR_ENCODE_PROCESS;
    if ((rc = get_scratch(5, (size_t)wsb, &d_ws))) return rc;
    if ((rc = get_scratch(4, (size_t)chunk * 64 + 1024, &d_aux))) return rc;
    int64_t* d_starts = reinterpret_cast<int64_t*>(d_aux);
    int64_t* d_nb = d_starts + chunk;
    float* d_q = reinterpret_cast<float*>(d_nb + chunk);
    float* d_off = d_q + chunk;
    float* d_gain = d_off + chunk;
    double* d_q64 = reinterpret_cast<double*>(d_nb + chunk);  // (the float64 form uses the same region: three doubles per stream)
    double* d_off64 = d_q64 + chunk;
    double* d_gain64 = d_off64 + chunk;
    int64_t* d_mm = reinterpret_cast<int64_t*>(d_gain64 + chunk);  // encode verification: first mismatch per stream
    unsigned char* d_dig = reinterpret_cast<unsigned char*>(d_mm + chunk);  // signing: the chunk's digests (16-byte aligned: d_aux is, chunk * 48 is)
    std::vector<int64_t> h_mm(verifying ? (size_t)chunk : 0);
    const int64_t cap_chunk = per_chunk.capacity;
    if ((rc = get_scratch(3, (size_t)cap_chunk + 256, &d_out))) return rc;
    if (((f32 && !fused_f32) || f64) && (rc = get_scratch(11, in_b + 256, &d_int))) return rc;

    // the blob: worst case reserved (address space only), populated ahead of the copies, trimmed at the end
    const int64_t cap_total = n_stream * one.capacity + 64;
    unsigned char* blob = reinterpret_cast<unsigned char*>(std::malloc((size_t)cap_total));
    bool reserved = (blob != nullptr);
    if (!reserved) {  // no overcommit: fall back to growing the blob chunk by chunk
        blob = reinterpret_cast<unsigned char*>(std::malloc(1));
        if (!blob) return FA_ERROR_ALLOC;
    }
    size_t blob_cap = reserved ? (size_t)cap_total : 1;
    FA_HTRACE("encode: buffers %.2f ms\n", (host_now() - t_enter) * 1e3);
    PagePopulator pop;
    // (what a typical array compresses to; the rest of the reservation stays untouched address space)
    if (reserved) pop.start(blob, std::min<size_t>((size_t)cap_total, (size_t)n_stream * stream_bytes / 8 * 5), 1, true);

    FA_HTRACE("encode: populate started %.2f ms\n", (host_now() - t_enter) * 1e3);
    Feeder feed;
    int err = FA_ERROR_NONE;
    if (n_chunks > 1) {
        err = feed.start(dev, n_chunks, [=](int64_t c, int slot, hipStream_t st) {
            const int64_t s0 = c * chunk, ns = std::min(chunk, n_stream - s0);
            if (hipMemcpyAsync(reinterpret_cast<char*>(d_in2) + (size_t)slot * in_slot, data + (size_t)s0 * stream_bytes, (size_t)ns * stream_bytes,
                               hipMemcpyHostToDevice, st) != hipSuccess) return (int)FA_ERROR_DEVICE;
            return (int)FA_ERROR_NONE;
        }, &ds_->feed_stream);
    }
    int64_t running = 0;
    FA_HTRACE("encode: set-up %.2f ms (entered at %.2f)\n", (host_now() - t_enter) * 1e3, t_enter * 1e3);
    for (int64_t c = 0; c < n_chunks && !err; ++c) {
        const int64_t s0 = c * chunk, ns = std::min(chunk, n_stream - s0);
        void* d_in = reinterpret_cast<char*>(d_in2) + (size_t)(c & 1) * in_slot;
        const double tw0 = host_now();
        if (n_chunks > 1) {
            if ((err = feed.wait_for(c))) break;
        } else if (hipMemcpy(d_in, data, (size_t)ns * stream_bytes, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        const double tw1 = host_now();
        int64_t total = 0;
        if (f32) {
            if (quanta && hipMemcpy(d_q, quanta + s0, (size_t)ns * 4, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
            const int32_t* ints = nullptr;
            if (fused_f32) {
                err = fa_encode_f32_device(reinterpret_cast<const float*>(d_in), ns, stream_size, level, quanta ? d_q : nullptr, d_ws, wsb,
                                           reinterpret_cast<unsigned char*>(d_out), cap_chunk, d_starts, d_nb, d_off, d_gain, &total, nullptr, nullptr);
            } else {
                err = fa_float32_to_int32_device(reinterpret_cast<const float*>(d_in), ns, stream_size, quanta ? d_q : nullptr,
                                                 reinterpret_cast<int32_t*>(d_int), d_off, d_gain, nullptr);
                ints = reinterpret_cast<const int32_t*>(d_int);
                if (!err) err = fa_encode_i32_device(ints, ns, stream_size, level, d_ws, wsb, reinterpret_cast<unsigned char*>(d_out), cap_chunk,
                                                     d_starts, d_nb, &total, nullptr, nullptr);
            }
            if (err) break;
            if (hipMemcpy(offsets + s0, d_off, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(gains + s0, d_gain, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        } else if (nch == 1) {
            err = fa_encode_i32_device(reinterpret_cast<const int32_t*>(d_in), ns, stream_size, level, d_ws, wsb,
                                       reinterpret_cast<unsigned char*>(d_out), cap_chunk, d_starts, d_nb, &total, nullptr, nullptr);
            if (err) break;
        } else {
            const void* src64 = d_in;
            if (f64) {
                if (quanta64 && hipMemcpy(d_q64, quanta64 + s0, (size_t)ns * 8, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
                err = fa_float64_to_int64_device(reinterpret_cast<const double*>(d_in), ns, stream_size, quanta64 ? d_q64 : nullptr,
                                                 reinterpret_cast<int64_t*>(d_int), d_off64, d_gain64, nullptr);
                if (err) break;
                if (hipMemcpy(offsets64 + s0, d_off64, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(gains64 + s0, d_gain64, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
                src64 = d_int;
            }
            err = fa_encode_i64_device(reinterpret_cast<const int64_t*>(src64), ns, stream_size, level, d_ws, wsb, reinterpret_cast<unsigned char*>(d_out),
                                       cap_chunk, d_starts, d_nb, &total, nullptr, nullptr);
            if (err) break;
        }
        if (verifying) {
            // decode what was just written and compare it with the input slot (float input through the offsets / gains the
            // encoder used): nothing crosses the link again but one word per stream
            const void *voff = nullptr, *vgain = nullptr;
            if (f32) { voff = d_off; vgain = d_gain; }
            if (f64) { voff = d_off64; vgain = d_gain64; }
            err = compare_device(nch, reinterpret_cast<const unsigned char*>(d_out), total, d_starts, d_nb, ns, stream_size, d_in, voff, vgain,
                                 d_mm, nullptr);
            if (!err && hipMemcpy(h_mm.data(), d_mm, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess) err = FA_ERROR_DEVICE;
            for (int64_t i = 0; i < ns && !err; ++i)
                if (h_mm[i] >= 0) err = FA_ERROR_ENCODE_VERIFY;
            if (err & (FA_ERROR_DECODE_INIT | FA_ERROR_DECODE_PROCESS | FA_ERROR_DECODE_SEEK))
                err = FA_ERROR_ENCODE_VERIFY;  // (a stream the decoder cannot read back is a failed verification)
            if (err) break;
        }
        if (signing) {
            // the STREAMINFO MD5 of the chunk's integers, hashed from the input slot while it is still there (float input is
            // quantised where it is loaded, with the offsets / gains the encoder used) and patched into the chunk's blob
            // before it goes down
            const void *soff = nullptr, *sgain = nullptr;
            if (f32) { soff = d_off; sgain = d_gain; }
            if (f64) { soff = d_off64; sgain = d_gain64; }
            err = md5_device(nch == 2, d_in, ns, stream_size, stream_size, soff, sgain, nullptr, 0, 1, d_dig, nullptr);
            if (!err) err = fa_sign_streams_device(reinterpret_cast<unsigned char*>(d_out), total, d_starts, ns, d_dig, nullptr);
            if (!err && hipStreamSynchronize(nullptr) != hipSuccess) err = FA_ERROR_DEVICE;
            if (err) break;
        }
        if (n_chunks > 1) {
            // The kernels are done with the input slot.  K3G and the slot sequence end with a stream synchronisation; K3F
            // returns with its finish kernels still queued, but those read the workspace and the blob only: K3F itself
            // and the short frames' encoder, the readers of the input, ran before its one wait.
            feed.done_with(c);
        }
        if ((size_t)(running + total) > blob_cap) {  // (only without the reservation)
            pop.join();
            unsigned char* nb2 = reinterpret_cast<unsigned char*>(std::realloc(blob, (size_t)(running + total)));
            if (!nb2) { err = FA_ERROR_ALLOC; break; }
            blob = nb2;
            blob_cap = (size_t)(running + total);
        }
        const double tw2 = host_now();
        if (hipMemcpy(blob + running, d_out, (size_t)total, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (hipMemcpy(starts + s0, d_starts, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        FA_HTRACE("encode chunk %lld: wait %.2f ms, kernels %.2f ms, download %.2f ms (%.1f MB) at %.2f\n", (long long)c, (tw1 - tw0) * 1e3,
                  (tw2 - tw1) * 1e3, (host_now() - tw2) * 1e3, total / 1e6, tw0 * 1e3);
        for (int64_t i = 0; i < ns; ++i) starts[s0 + i] += running;
        running += total;
    }
    const double tf0 = host_now();
    feed.finish();
    pop.join();
    FA_HTRACE("encode: joins %.2f ms\n", (host_now() - tf0) * 1e3);
    if (err) {
        std::free(blob);
        for (int64_t i = 0; i < n_stream; ++i) starts[i] = 0;
        return err;
    }
    // trim the reservation to the bytes written (a shrinking realloc of an mmap'd block returns its tail to the system)
    const double tr0 = host_now();
    unsigned char* fit = reinterpret_cast<unsigned char*>(std::realloc(blob, running > 0 ? (size_t)running : 1));
    FA_HTRACE("encode: trim %.2f ms, whole call %.2f ms\n", (host_now() - tr0) * 1e3, (host_now() - t_enter) * 1e3);
    *bytes = fit ? fit : blob;
    *n_bytes = running;
    return FA_ERROR_NONE;
}

int fa_encode_f32_host(const float* data, int64_t n_stream, int64_t stream_size, uint32_t level, const float* quanta, int64_t* n_bytes,
                       int64_t* starts, unsigned char** bytes, float* offsets, float* gains) {
    if (!offsets || !gains) return FA_ERROR_CONVERT_TYPE;
    return encode_host(data, 1, n_stream, stream_size, level, n_bytes, starts, bytes, true, quanta, offsets, gains);
}

int fa_encode_f64_host(const double* data, int64_t n_stream, int64_t stream_size, uint32_t level, const double* quanta, int64_t* n_bytes,
                       int64_t* starts, unsigned char** bytes, double* offsets, double* gains) {
    if (!offsets || !gains) return FA_ERROR_CONVERT_TYPE;
    return encode_host(data, 2, n_stream, stream_size, level, n_bytes, starts, bytes, false, nullptr, nullptr, nullptr, true, quanta, offsets, gains);
}

int encode_i32(int32_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
               int64_t* starts, unsigned char** bytes) {
    return encode_host(data, 1, n_stream, stream_size, level, n_bytes, starts, bytes);
}

int encode_i32_threaded(int32_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
                        int64_t* starts, unsigned char** bytes) {
    return encode_host(data, 1, n_stream, stream_size, level, n_bytes, starts, bytes);
}

int encode_i64(int64_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
               int64_t* starts, unsigned char** bytes) {
    return encode_host(reinterpret_cast<const int32_t*>(data), 2, n_stream, stream_size, level, n_bytes, starts, bytes);
}

int encode_i64_threaded(int64_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
                        int64_t* starts, unsigned char** bytes) {
    return encode_host(reinterpret_cast<const int32_t*>(data), 2, n_stream, stream_size, level, n_bytes, starts, bytes);
}

// One chunk of streams as the decoder wants it: the byte ranges of its streams, sorted and merged where they touch (or
// nearly touch), packed into one device buffer.  Only those ranges are uploaded -- a keep mask that selects a few
// streams of a large store moves the bytes of those streams, not everything between the first and the last.
struct ChunkRanges {
    struct Piece { int64_t src, len, dst; };
    std::vector<Piece> pieces;
    std::vector<int64_t> rel;  // start of every stream of the chunk inside the packed buffer
    int64_t packed = 0;
    bool ok = true;
    void build(const int64_t* starts, const int64_t* nbytes, int64_t s0, int64_t ns) {
        pieces.clear();
        rel.assign((size_t)ns, 0);
        packed = 0;
        ok = true;
        std::vector<int64_t> order((size_t)ns);
        for (int64_t i = 0; i < ns; ++i) {
            order[(size_t)i] = i;
            // the C signature carries no blob length: negative or overflowing entries are all that can be refused here
            if (starts[s0 + i] < 0 || nbytes[s0 + i] < 0 || starts[s0 + i] > INT64_MAX - nbytes[s0 + i]) ok = false;
        }
        if (!ok) return;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return starts[s0 + a] < starts[s0 + b]; });
        int64_t lo = -1, hi = -1;
        auto flush = [&]() {
            if (lo < 0) return;
            pieces.push_back({lo, hi - lo, packed});
            packed += (hi - lo + 255) / 256 * 256;  // every piece starts 256-byte aligned
        };
        std::vector<int64_t> piece_of((size_t)ns);
        for (int64_t k = 0; k < ns; ++k) {
            const int64_t i = order[(size_t)k], a = starts[s0 + i], b = a + nbytes[s0 + i];
            if (lo >= 0 && a <= hi + 4096) {
                if (b > hi) hi = b;
            } else {
                flush();
                lo = a; hi = b;
            }
            piece_of[(size_t)i] = (int64_t)pieces.size();  // (index of the piece being built)
        }
        flush();
        if (pieces.size() > 2048) {  // too scattered for one copy per piece: everything between the first and the last byte
            const int64_t a = pieces.front().src, b = pieces.back().src + pieces.back().len;
            pieces.assign(1, {a, b - a, 0});
            packed = b - a;
            for (int64_t i = 0; i < ns; ++i) rel[(size_t)i] = starts[s0 + i] - a;
            return;
        }
        for (int64_t i = 0; i < ns; ++i) {
            const Piece& pc = pieces[(size_t)piece_of[(size_t)i]];
            rel[(size_t)i] = pc.dst + (starts[s0 + i] - pc.src);
        }
    }
};

// offsets / gains (both or neither; float for one channel, double for two): the int -> float restore (utils.c:329-368) is
// fused into the decoder's store and `data_v` receives float32 / float64 -- the integers never cross PCIe.
static int decode_host(const unsigned char* bytes, const int64_t* starts, const int64_t* nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first_sample, int64_t last_sample, void* data_v, int nch,
                       const void* offsets = nullptr, const void* gains = nullptr) {
    FA_API_LOCK;
    const double t_enter = host_now();
    const size_t esz = 4 * (size_t)nch;  // bytes per decoded sample
    unsigned char* data = reinterpret_cast<unsigned char*>(data_v);
    int64_t first_decode, n_decode;
    int rc = validate_range(stream_size, first_sample, last_sample, &first_decode, &n_decode);  // decompress.c:209-222
    if (rc) return rc;
    if (n_stream <= 0) return FA_ERROR_NONE;
    if (fa_device_count() <= 0) return FA_ERROR_DEVICE;
    int dev = 0;
    FA_HIP_TRY(hipGetDevice(&dev));
    // The reference's decoder always checks the frame CRC-16 (libFLAC reports a mismatch through the error callback,
    // decompress.c:104-121); on this entry point the check is on unless FLACARRAY_HIP_HOST_VERIFY=0 -- the bytes
    // crossed PCIe anyway, one more read of them in HBM is in the noise.
    const char* hv = std::getenv("FLACARRAY_HIP_HOST_VERIFY");
    const int host_verify = (hv && hv[0] == '0') ? 0 : 1;
    const size_t row_bytes = (size_t)n_decode * esz;
    // Chunks are bounded on BOTH sides: by decoded bytes (~256 MiB of output) and by the compressed bytes of their
    // streams (~256 MiB of input) -- a short sample range over a large store (arr[:, 0:100]) has tiny rows and would
    // otherwise put the whole store into one chunk.  Device memory in use: two input slots (one when there is a single
    // chunk) + one output chunk, whatever the store's size.
    const int64_t chunk = host_chunk_streams(n_stream, row_bytes, 0x7fffffffLL);  // (streams per chunk by output bytes)
    int64_t in_target = 256ll << 20;
    if (const char* e = std::getenv("FLACARRAY_HIP_HOST_CHUNK_BYTES")) {
        const long long v = std::atoll(e);
        if (v > 0) in_target = v;
    }
    std::vector<int64_t> cb;  // chunk c = streams [cb[c], cb[c + 1])
    cb.push_back(0);
    {
        int64_t in_sum = 0;
        for (int64_t s = 0; s < n_stream; ++s) {
            const int64_t nbs = nbytes[s] > 0 ? nbytes[s] : 0;
            if (s > cb.back() && (s - cb.back() >= chunk || in_sum + nbs > in_target)) { cb.push_back(s); in_sum = 0; }
            in_sum += nbs;
        }
        cb.push_back(n_stream);
    }
    const int64_t n_chunks = (int64_t)cb.size() - 1;

    // byte ranges of every chunk (host side, cheap), and the largest packed size: the upload slots are that large
    std::vector<ChunkRanges> cr((size_t)n_chunks);
    int64_t max_packed = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t s0 = cb[(size_t)c], ns = cb[(size_t)c + 1] - s0;
        cr[(size_t)c].build(starts, nbytes, s0, ns);
        if (!cr[(size_t)c].ok || cr[(size_t)c].packed <= 0) return FA_ERROR_DECODE_INIT;
        max_packed = std::max(max_packed, cr[(size_t)c].packed);
    }
    void *d_blob2 = nullptr, *d_aux2 = nullptr, *d_out = nullptr;
    const size_t blob_slot = align_up((size_t)max_packed + 256, 256);
    const size_t aux_slot = align_up((size_t)chunk * 32 + 512, 256);  // starts, nbytes, (offsets, gains: up to 8 B each)
    int err = FA_ERROR_NONE;
    if ((err = get_scratch(0, (n_chunks > 1 ? 2 : 1) * blob_slot, &d_blob2))) return err;
    if ((err = get_scratch(4, 2 * aux_slot, &d_aux2))) return err;
    if ((err = get_scratch(5, (size_t)chunk * row_bytes * (nch == 2 ? 1 : 1) + 256, &d_out))) return err;

    // the caller's output array is usually fresh memory (np.empty): populate its pages beside the first upload
    FA_HTRACE("decode: buffers %.2f ms\n", (host_now() - t_enter) * 1e3);
    PagePopulator pop;
    pop.start(data, (size_t)n_stream * row_bytes, 1, false);
    FA_HTRACE("decode: populate started %.2f ms\n", (host_now() - t_enter) * 1e3);

    auto upload = [&, bytes, nbytes](int64_t c, int slot, hipStream_t st) -> int {
        const int64_t s0 = cb[(size_t)c], ns = cb[(size_t)c + 1] - s0;
        const ChunkRanges& r = cr[(size_t)c];
        char* db = reinterpret_cast<char*>(d_blob2) + (size_t)slot * blob_slot;
        for (const auto& pc : r.pieces)
            if (hipMemcpyAsync(db + pc.dst, bytes + pc.src, (size_t)pc.len, hipMemcpyHostToDevice, st) != hipSuccess) return FA_ERROR_DEVICE;
        char* da = reinterpret_cast<char*>(d_aux2) + (size_t)slot * aux_slot;
        if (hipMemcpyAsync(da, r.rel.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st) != hipSuccess) return FA_ERROR_DEVICE;
        if (hipMemcpyAsync(da + (size_t)chunk * 8, nbytes + s0, (size_t)ns * 8, hipMemcpyHostToDevice, st) != hipSuccess) return FA_ERROR_DEVICE;
        if (offsets) {
            const size_t fsz = (nch == 2) ? 8 : 4;
            if (hipMemcpyAsync(da + (size_t)chunk * 16, reinterpret_cast<const char*>(offsets) + (size_t)s0 * fsz, (size_t)ns * fsz, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipMemcpyAsync(da + (size_t)chunk * 24, reinterpret_cast<const char*>(gains) + (size_t)s0 * fsz, (size_t)ns * fsz, hipMemcpyHostToDevice, st) != hipSuccess)
                return FA_ERROR_DEVICE;
        }
        return FA_ERROR_NONE;
    };
    Feeder feed;
    if (n_chunks > 1) err = feed.start(dev, n_chunks, upload, &ds_->feed_stream);
    FA_HTRACE("decode: set-up %.2f ms (entered at %.2f)\n", (host_now() - t_enter) * 1e3, t_enter * 1e3);
    for (int64_t c = 0; c < n_chunks && !err; ++c) {
        const int64_t s0 = cb[(size_t)c], ns = cb[(size_t)c + 1] - s0;
        const int slot = (int)(c & 1);
        if (n_chunks > 1) {
            if ((err = feed.wait_for(c))) break;
        } else {
            if ((err = upload(0, 0, nullptr))) break;
            if (hipStreamSynchronize(nullptr) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        }
        const unsigned char* db = reinterpret_cast<const unsigned char*>(d_blob2) + (size_t)slot * blob_slot;
        const int64_t* d_starts = reinterpret_cast<const int64_t*>(reinterpret_cast<char*>(d_aux2) + (size_t)slot * aux_slot);
        const int64_t* d_nb = d_starts + chunk;
        const int64_t packed = cr[(size_t)c].packed;
        const char* d_fo = reinterpret_cast<const char*>(d_starts) + (size_t)chunk * 16;  // offsets, gains of the chunk (if any)
        const char* d_fg = reinterpret_cast<const char*>(d_starts) + (size_t)chunk * 24;
        DecodeRequest rq;
        rq.nch = nch; rq.first = first_decode; rq.n_decode = n_decode; rq.verify = host_verify;
        if (offsets) rq.output(nullptr, d_out, d_fo, d_fg); else rq.out_int = d_out;
        err = decode_device_impl(rq.store(db, packed, d_starts, d_nb, ns, stream_size));
        if (n_chunks > 1) feed.done_with(c);  // (the decode call ends with a stream synchronisation: the slot is free)
        if (err) break;
        const double td0 = host_now();
        if (hipMemcpy(data + (size_t)s0 * row_bytes, d_out, (size_t)ns * row_bytes, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        FA_HTRACE("decode chunk %lld: download %.2f ms at %.2f\n", (long long)c, (host_now() - td0) * 1e3, td0 * 1e3);
    }
    const double tj0 = host_now();
    feed.finish();
    pop.join();
    FA_HTRACE("decode: joins %.2f ms, whole call %.2f ms\n", (host_now() - tj0) * 1e3, (host_now() - t_enter) * 1e3);
    return err;
}

int decode_i32(unsigned char* const bytes, int64_t* const starts, int64_t* const nbytes, int64_t n_stream,
               int64_t stream_size, int64_t first_sample, int64_t last_sample, int32_t* data, bool use_threads) {
    (void)use_threads;
    return decode_host(bytes, starts, nbytes, n_stream, stream_size, first_sample, last_sample, data, 1);
}

int decode_i64(unsigned char* const bytes, int64_t* const starts, int64_t* const nbytes, int64_t n_stream,
               int64_t stream_size, int64_t first_sample, int64_t last_sample, int64_t* data, bool use_threads) {
    (void)use_threads;
    return decode_host(bytes, starts, nbytes, n_stream, stream_size, first_sample, last_sample, data, 2);
}

int fa_decode_f32_host(const unsigned char* bytes, const int64_t* starts, const int64_t* nbytes, int64_t n_stream, int64_t stream_size,
                       int64_t first_sample, int64_t last_sample, const float* offsets, const float* gains, float* data) {
    if (!offsets || !gains) return FA_ERROR_CONVERT_TYPE;
    return decode_host(bytes, starts, nbytes, n_stream, stream_size, first_sample, last_sample, data, 1, offsets, gains);
}

int fa_decode_f64_host(const unsigned char* bytes, const int64_t* starts, const int64_t* nbytes, int64_t n_stream, int64_t stream_size,
                       int64_t first_sample, int64_t last_sample, const double* offsets, const double* gains, double* data) {
    if (!offsets || !gains) return FA_ERROR_CONVERT_TYPE;
    return decode_host(bytes, starts, nbytes, n_stream, stream_size, first_sample, last_sample, data, 2, offsets, gains);
}

int float32_to_int32(float const* input, int64_t n_stream, int64_t stream_size, float const* quanta, int32_t* output,
                     float* offsets, float* gains) {
    FA_API_LOCK;
    if (n_stream <= 0 || stream_size <= 0) return FA_ERROR_NONE;
    if (fa_device_count() <= 0) return FA_ERROR_DEVICE;
    size_t free_b = 0, total_b = 0;
    FA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    int64_t chunk = (int64_t)((free_b / 10 * 8) / ((size_t)stream_size * 8 + 64));
    if (chunk < 1) chunk = 1;
    if (chunk > n_stream) chunk = n_stream;
    int err = FA_ERROR_NONE;
    for (int64_t s0 = 0; s0 < n_stream && !err; s0 += chunk) {
        const int64_t ns = (n_stream - s0 < chunk) ? (n_stream - s0) : chunk;
        const size_t nb = (size_t)ns * (size_t)stream_size * 4;
        void *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
        if ((err = get_scratch(0, nb, &d_in))) break;
        if ((err = get_scratch(5, nb, &d_out))) break;
        if ((err = get_scratch(3, (size_t)ns * 12 + 768, &d_aux))) break;
        float* d_q = reinterpret_cast<float*>(d_aux);
        float* d_off = d_q + ns;
        float* d_gain = d_off + ns;
        if (hipMemcpy(d_in, input + s0 * stream_size, nb, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (quanta && hipMemcpy(d_q, quanta + s0, (size_t)ns * 4, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        err = fa_float32_to_int32_device(reinterpret_cast<const float*>(d_in), ns, stream_size, quanta ? d_q : nullptr,
                                         reinterpret_cast<int32_t*>(d_out), d_off, d_gain, nullptr);
        if (err) break;
        if (hipMemcpy(output + s0 * stream_size, d_out, nb, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (hipMemcpy(offsets + s0, d_off, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (hipMemcpy(gains + s0, d_gain, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
    }
    return err;
}

void int32_to_float32(int32_t const* input, int64_t n_stream, int64_t stream_size, float const* offsets,
                      float const* gains, float* output) {
    FA_API_LOCK_OR(fatal_device("int32_to_float32", "hipGetDevice"));
    if (n_stream <= 0 || stream_size <= 0) return;
    if (fa_device_count() <= 0) fatal_device("int32_to_float32", "hipGetDeviceCount (no HIP device)");
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) fatal_device("int32_to_float32", "hipMemGetInfo");
    int64_t chunk = (int64_t)((free_b / 10 * 8) / ((size_t)stream_size * 8 + 64));
    if (chunk < 1) chunk = 1;
    if (chunk > n_stream) chunk = n_stream;
    for (int64_t s0 = 0; s0 < n_stream; s0 += chunk) {
        const int64_t ns = (n_stream - s0 < chunk) ? (n_stream - s0) : chunk;
        const size_t nb = (size_t)ns * (size_t)stream_size * 4;
        void *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
        const char* fn = "int32_to_float32";
        if (get_scratch(0, nb, &d_in) || get_scratch(5, nb, &d_out) || get_scratch(3, (size_t)ns * 8 + 512, &d_aux))
            fatal_device(fn, "hipMalloc of the staging buffers");
        float* d_off = reinterpret_cast<float*>(d_aux);
        float* d_gain = d_off + ns;
        if (hipMemcpy(d_in, input + s0 * stream_size, nb, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(input, H2D)");
        if (hipMemcpy(d_off, offsets + s0, (size_t)ns * 4, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(offsets, H2D)");
        if (hipMemcpy(d_gain, gains + s0, (size_t)ns * 4, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(gains, H2D)");
        if (fa_int32_to_float32_device(reinterpret_cast<const int32_t*>(d_in), ns, stream_size, d_off, d_gain,
                                       reinterpret_cast<float*>(d_out), nullptr) != FA_ERROR_NONE)
            fatal_device(fn, "int32_to_float32_kernel launch");
        if (hipMemcpy(output + s0 * stream_size, d_out, nb, hipMemcpyDeviceToHost) != hipSuccess) fatal_device(fn, "hipMemcpy(output, D2H)");
    }
}

int float64_to_int64(double const* input, int64_t n_stream, int64_t stream_size, double const* quanta, int64_t* output,
                     double* offsets, double* gains) {
    FA_API_LOCK;
    if (n_stream <= 0 || stream_size <= 0) return FA_ERROR_NONE;
    if (fa_device_count() <= 0) return FA_ERROR_DEVICE;
    size_t free_b = 0, total_b = 0;
    FA_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    int64_t chunk = (int64_t)((free_b / 10 * 8) / ((size_t)stream_size * 16 + 64));
    if (chunk < 1) chunk = 1;
    if (chunk > n_stream) chunk = n_stream;
    int err = FA_ERROR_NONE;
    for (int64_t s0 = 0; s0 < n_stream && !err; s0 += chunk) {
        const int64_t ns = (n_stream - s0 < chunk) ? (n_stream - s0) : chunk;
        const size_t nb = (size_t)ns * (size_t)stream_size * 8;
        void *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
        if ((err = get_scratch(0, nb, &d_in))) break;
        if ((err = get_scratch(5, nb, &d_out))) break;
        if ((err = get_scratch(3, (size_t)ns * 24 + 768, &d_aux))) break;
        double* d_q = reinterpret_cast<double*>(d_aux);
        double* d_off = d_q + ns;
        double* d_gain = d_off + ns;
        if (hipMemcpy(d_in, input + s0 * stream_size, nb, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (quanta && hipMemcpy(d_q, quanta + s0, (size_t)ns * 8, hipMemcpyHostToDevice) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        err = fa_float64_to_int64_device(reinterpret_cast<const double*>(d_in), ns, stream_size, quanta ? d_q : nullptr,
                                         reinterpret_cast<int64_t*>(d_out), d_off, d_gain, nullptr);
        if (err) break;
        if (hipMemcpy(output + s0 * stream_size, d_out, nb, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (hipMemcpy(offsets + s0, d_off, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
        if (hipMemcpy(gains + s0, d_gain, (size_t)ns * 8, hipMemcpyDeviceToHost) != hipSuccess) { err = FA_ERROR_DEVICE; break; }
    }
    return err;
}

void int64_to_float64(int64_t const* input, int64_t n_stream, int64_t stream_size, double const* offsets,
                      double const* gains, double* output) {
    FA_API_LOCK_OR(fatal_device("int64_to_float64", "hipGetDevice"));
    if (n_stream <= 0 || stream_size <= 0) return;
    if (fa_device_count() <= 0) fatal_device("int64_to_float64", "hipGetDeviceCount (no HIP device)");
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) fatal_device("int64_to_float64", "hipMemGetInfo");
    int64_t chunk = (int64_t)((free_b / 10 * 8) / ((size_t)stream_size * 16 + 64));
    if (chunk < 1) chunk = 1;
    if (chunk > n_stream) chunk = n_stream;
    for (int64_t s0 = 0; s0 < n_stream; s0 += chunk) {
        const int64_t ns = (n_stream - s0 < chunk) ? (n_stream - s0) : chunk;
        const size_t nb = (size_t)ns * (size_t)stream_size * 8;
        void *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
        const char* fn = "int64_to_float64";
        if (get_scratch(0, nb, &d_in) || get_scratch(5, nb, &d_out) || get_scratch(3, (size_t)ns * 16 + 512, &d_aux))
            fatal_device(fn, "hipMalloc of the staging buffers");
        double* d_off = reinterpret_cast<double*>(d_aux);
        double* d_gain = d_off + ns;
        if (hipMemcpy(d_in, input + s0 * stream_size, nb, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(input, H2D)");
        if (hipMemcpy(d_off, offsets + s0, (size_t)ns * 8, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(offsets, H2D)");
        if (hipMemcpy(d_gain, gains + s0, (size_t)ns * 8, hipMemcpyHostToDevice) != hipSuccess) fatal_device(fn, "hipMemcpy(gains, H2D)");
        if (fa_int64_to_float64_device(reinterpret_cast<const int64_t*>(d_in), ns, stream_size, d_off, d_gain,
                                       reinterpret_cast<double*>(d_out), nullptr) != FA_ERROR_NONE)
            fatal_device(fn, "int64_to_float64_kernel launch");
        if (hipStreamSynchronize(nullptr) != hipSuccess) fatal_device(fn, "hipStreamSynchronize");
        if (hipMemcpy(output + s0 * stream_size, d_out, nb, hipMemcpyDeviceToHost) != hipSuccess) fatal_device(fn, "hipMemcpy(output, D2H)");
    }
}

}  // extern "C"
