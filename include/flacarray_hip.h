/*
 * flacarray_hip.h -- C ABI of the MI355X-native FLAC encode/decode path.
 *
 * The first group of entry points has exactly the names, argument lists, return codes and
 * ownership rules of the reference's C layer, so the reference's Cython binding
 * (src/flacarray/libflacarray/libflacarray.pyx:18-110 `cdef extern from "flacarray.h"`) can be
 * linked against libflacarray_hip.so instead of compress.c/decompress.c/utils.c + libFLAC.
 * The second group takes DEVICE pointers (data already resident in HBM) and is what the
 * Python layer, the tests and bench.py use.
 *
 * No torch / HIP types appear in any signature: `void* stream` is a hipStream_t passed as an
 * opaque pointer (NULL = default stream).
 */
#ifndef FLACARRAY_HIP_H
#define FLACARRAY_HIP_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error bit-codes, identical to the reference (src/flacarray/libflacarray/flacarray.h:20-40). */
#define FA_ERROR_NONE 0
#define FA_ERROR_ALLOC (1 << 0)
#define FA_ERROR_INVALID_LEVEL (1 << 1)
#define FA_ERROR_ZERO_NSTREAM (1 << 2)
#define FA_ERROR_ZERO_STREAMSIZE (1 << 3)
#define FA_ERROR_ENCODE_INIT (1 << 8)
#define FA_ERROR_ENCODE_PROCESS (1 << 9)
#define FA_ERROR_DECODE_INIT (1 << 13)
#define FA_ERROR_DECODE_PROCESS (1 << 14)
#define FA_ERROR_DECODE_STREAMSIZE (1 << 16)
#define FA_ERROR_DECODE_SAMPLE_RANGE (1 << 17)
#define FA_ERROR_DECODE_SEEK (1 << 18)
#define FA_ERROR_CONVERT_TYPE (1 << 19)
/* additions of this library */
#define FA_ERROR_DEVICE (1 << 24)   /* a HIP runtime call failed (no GPU, out of memory, ...) */
#define FA_ERROR_NAN_INPUT (1 << 25) /* float32_to_int32 saw a NaN */
#define FA_ERROR_ENCODE_VERIFY (1 << 26) /* encode verification: a stream does not decode to its input (fa_set_encode_verify) */

/* ---------------------------------------------------------------------------------------
 * Group 1: host-pointer drop-ins for the reference C ABI
 * ------------------------------------------------------------------------------------- */

/* replaces encode_i32, flacarray.h:209-217 (compress.c:440).  `*bytes` is malloc()'d by the
 * callee and owned by the caller (free()), as in compress.c:251,414. */
int encode_i32(int32_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
               int64_t* starts, unsigned char** bytes);

/* replaces encode_i32_threaded, flacarray.h:219-227 (compress.c:461); same work on the GPU */
int encode_i32_threaded(int32_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
                        int64_t* starts, unsigned char** bytes);

/* replaces decode_i32, flacarray.h:249-259 (decompress.c:318).  first_sample/last_sample < 0
 * decodes whole streams; otherwise the half-open range [first_sample, last_sample) of every
 * stream, row stride last_sample-first_sample (decompress.c:209-222,254). */
int decode_i32(unsigned char* const bytes, int64_t* const starts, int64_t* const nbytes, int64_t n_stream,
               int64_t stream_size, int64_t first_sample, int64_t last_sample, int32_t* data, bool use_threads);

/* replace encode_i64 / encode_i64_threaded, flacarray.h:229-247 (compress.c:482-540): int64 samples
 * as two-channel 32-bit streams, channel 0 = low word, channel 1 = high word (utils.c:96-123); the
 * channels are coded independently (channel assignment "left/right") */
int encode_i64(int64_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
               int64_t* starts, unsigned char** bytes);
int encode_i64_threaded(int64_t* const data, int64_t n_stream, int64_t stream_size, uint32_t level, int64_t* n_bytes,
                        int64_t* starts, unsigned char** bytes);

/* replaces decode_i64, flacarray.h:261-271 (decompress.c:343-375): two-channel streams, int64
 * sample = (channel 1 << 32) | (channel 0 as unsigned) (utils.c:96-123).  Reads streams with any
 * stereo channel assignment (left/right, left/side, side/right, mid/side). */
int decode_i64(unsigned char* const bytes, int64_t* const starts, int64_t* const nbytes, int64_t n_stream,
               int64_t stream_size, int64_t first_sample, int64_t last_sample, int64_t* data, bool use_threads);

/* replaces float32_to_int32, flacarray.h:275-283 (utils.c:160); quanta == NULL: per-stream
 * quanta from the data range */
int float32_to_int32(float const* input, int64_t n_stream, int64_t stream_size, float const* quanta, int32_t* output,
                     float* offsets, float* gains);

/* replaces int32_to_float32, flacarray.h:304-311 (utils.c:350) */
void int32_to_float32(int32_t const* input, int64_t n_stream, int64_t stream_size, float const* offsets,
                      float const* gains, float* output);

/* replace float64_to_int64 / int64_to_float64, flacarray.h:285-302 (utils.c:245-348) */
int float64_to_int64(double const* input, int64_t n_stream, int64_t stream_size, double const* quanta, int64_t* output,
                     double* offsets, double* gains);
void int64_to_float64(int64_t const* input, int64_t n_stream, int64_t stream_size, double const* offsets,
                      double const* gains, double* output);

/* ---------------------------------------------------------------------------------------
 * Group 2: device-pointer entry points (every pointer named d_* is HBM memory)
 * ------------------------------------------------------------------------------------- */

/* bytes of scratch fa_encode_i32_device_begin needs for this problem size */
int64_t fa_encode_workspace_bytes(int64_t n_stream, int64_t stream_size, uint32_t level);

/* Encode, phase 1: analyse and bit-pack every frame into the workspace, size the output.
 * Writes d_starts[n_stream], d_nbytes[n_stream] (device) and *h_total_bytes (host; the call
 * synchronises the stream to deliver it).  d_info may be NULL; otherwise it receives 8 int32
 * per frame {type, order, partition order, wasted bits, shift, precision, bytes, blocksize}. */
int fa_encode_i32_device_begin(const int32_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level,
                               void* d_workspace, int64_t workspace_bytes, int64_t* d_starts, int64_t* d_nbytes,
                               int64_t* h_total_bytes, int32_t* d_info, void* stream);

/* Encode, phase 2: assemble the blob (stream headers, byte-exact concatenation, CRC-16) into
 * d_bytes[*h_total_bytes].  Same arguments as phase 1. */
int fa_encode_i32_device_finish(int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                                const int64_t* d_starts, unsigned char* d_bytes, void* stream);

/* Single-pass encode: ONE kernel analyses every frame, sizes it, obtains its byte offset from a look-back over the frames
 * before it (a scanner wave turns published sizes into offsets) and the frame ends up -- CRC-16 included -- at its final
 * place in d_bytes; no K4 scans, no K5 pass, no size read-back before the blob is written.  Two kernels share the work:
 *   K3F  levels 3-8, 16-byte aligned rows, stream_size a multiple of 4096 -- or a multiple of 4 and at least 8192, in which
 *        case every stream's short last frame takes a detour through a slot: the bitstream is written straight from the
 *        wave's registers, there are no slots;
 *   K3G  everything else (levels 0-2 = 1152-sample blocks, streams shorter than two frames, any length, unaligned rows,
 *        and -- fa_encode_i64_device -- the two-channel frames of int64 arrays): K3's frame body packs the frame into
 *        the wave's own slot (a few thousand slots in all, cache resident) and the wave moves it once its offset is known.
 * fa_encode_single_pass_supported is 1 for every valid geometry (0 only under FLACARRAY_HIP_SLOTS, the diagnostic switch
 * that sends everything through begin + finish).  The caller provides d_bytes with fa_encode_capacity_bytes() bytes
 * (worst case: every frame VERBATIM; a smaller buffer is accepted -- if the blob does not fit, nothing outside the
 * buffer is written and the call returns FA_ERROR_ALLOC) and a workspace of fa_encode_single_pass_workspace_bytes(); the
 * encoded triple is d_bytes[0, *h_total_bytes), d_starts, d_nbytes.  Same bytes as begin + finish in every case.
 * The call waits on `stream` once (for the error word and the total, which is valid on return); d_bytes / d_starts / d_nbytes
 * are complete in stream order: K3F's header and index kernel may still be queued when the call returns. */
int fa_encode_single_pass_supported(int64_t n_stream, int64_t stream_size, uint32_t level);
int64_t fa_encode_capacity_bytes(int64_t n_stream, int64_t stream_size, uint32_t level);
int64_t fa_encode_single_pass_workspace_bytes(int64_t n_stream, int64_t stream_size, uint32_t level);
int fa_encode_i32_device(const int32_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                         int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info, void* stream);

/* float32 input, quantisation fused into the single-pass encoder (float32_to_int32 of utils.c:160-243 without the
 * int32 round trip through HBM): a range pre-pass writes d_offsets / d_gains[n_stream] (d_quanta may be NULL = per-stream
 * quanta from the data range), then the encoder quantises every sample where it loads it.  Same bytes, offsets and
 * gains as fa_float32_to_int32_device followed by fa_encode_i32_device.  Only for geometries the single-pass kernel
 * covers (fa_encode_single_pass_supported); FA_ERROR_ENCODE_INIT otherwise, FA_ERROR_NAN_INPUT for a NaN. */
int fa_encode_f32_device(const float* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, const float* d_quanta,
                         void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes,
                         int64_t* d_starts, int64_t* d_nbytes, float* d_offsets, float* d_gains, int64_t* h_total_bytes,
                         int32_t* d_info, void* stream);

/* Host-pointer form of the fused float32 path: what array_compress does with float32 input (compress.py:50-84:
 * float_to_int, then encode_flac) in ONE pass over PCIe -- the float32 samples go up once, are quantised where the
 * encoder loads them (fa_encode_f32_device; geometries the single-pass kernel does not cover are quantised on the device
 * first), and only the compressed bytes come back.  quanta may be NULL (per-stream quanta from the data range) or
 * hold n_stream values; offsets / gains [n_stream] are outputs; *bytes is malloc()'d as in encode_i32.
 * FA_ERROR_NAN_INPUT for a NaN. */
int fa_encode_f32_host(const float* data, int64_t n_stream, int64_t stream_size, uint32_t level, const float* quanta,
                       int64_t* n_bytes, int64_t* starts, unsigned char** bytes, float* offsets, float* gains);

/* The float64 twin: what array_compress does with float64 input -- float64_to_int64 (utils.c:245-327) followed by
 * encode_i64 (compress.py:50-84) -- in one trip: the float64 samples go up once, are quantised on the device and encoded
 * from there as two-channel streams; the int64 image never crosses PCIe (the two-call form moves 8 B per sample down and
 * up again).  quanta may be NULL; offsets / gains [n_stream] are outputs.  FA_ERROR_NAN_INPUT for a NaN. */
int fa_encode_f64_host(const double* data, int64_t n_stream, int64_t stream_size, uint32_t level, const double* quanta,
                       int64_t* n_bytes, int64_t* starts, unsigned char** bytes, double* offsets, double* gains);

/* Decode with the int -> float restore fused into the decoder's store: what array_decompress_slice does for float data
 * (decode_flac, then int_to_float: decompress.py:107-136, utils.c:329-368) in one trip -- compressed bytes up, floats
 * down; the integers never cross PCIe.  offsets / gains [n_stream] as float_to_int returned them; data is
 * float32 / float64 [n_stream][n_decode]; sample range and error codes as decode_i32 / decode_i64 (frame CRC-16s checked). */
int fa_decode_f32_host(const unsigned char* bytes, const int64_t* starts, const int64_t* nbytes, int64_t n_stream, int64_t stream_size,
                       int64_t first_sample, int64_t last_sample, const float* offsets, const float* gains, float* data);
int fa_decode_f64_host(const unsigned char* bytes, const int64_t* starts, const int64_t* nbytes, int64_t n_stream, int64_t stream_size,
                       int64_t first_sample, int64_t last_sample, const double* offsets, const double* gains, double* data);

/* The same three calls for int64 input (two-channel streams); d_info, if given, holds one
 * FrameInfo per SUBFRAME: [ (stream * frames + frame) * 2 + channel ]. */
int64_t fa_encode_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level);
int fa_encode_i64_device_begin(const int64_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level,
                               void* d_workspace, int64_t workspace_bytes, int64_t* d_starts, int64_t* d_nbytes,
                               int64_t* h_total_bytes, int32_t* d_info, void* stream);
int fa_encode_i64_device_finish(int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                                const int64_t* d_starts, unsigned char* d_bytes, void* stream);
/* ... and the single-pass form (K3G; replaces FLAC__stream_encoder_process_interleaved on two channels,
 * compress.c:482-540) with its capacity and workspace queries. */
int64_t fa_encode_capacity_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level);
int64_t fa_encode_single_pass_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, uint32_t level);
int fa_encode_i64_device(const int64_t* d_data, int64_t n_stream, int64_t stream_size, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                         int64_t* d_nbytes, int64_t* h_total_bytes, int32_t* d_info, void* stream);

/* Append: extend every stream of a device-resident store (written by this library: one SEEKTABLE point per frame) by
 * n samples -- d_data[n_stream][n], int32 for one-channel streams (fa_append_i32_device), int64 for two-channel streams
 * (fa_append_i64_device) -- so that the result is, byte for byte, what fa_encode_i32_device / fa_encode_i64_device writes for
 * the concatenation (same level: its block size must be the one in the streams' STREAMINFO).  The old short last frame of
 * every stream is decoded, the (n_stream, r + n) image of it and the new samples is encoded, and one splice kernel (the one
 * fa_overwrite_*_device runs: the span is the old short last frame, nothing lies behind it and the stream grows) writes the
 * result: a new stream header, the kept old frames verbatim, the new frames renumbered (UTF-8 frame number, CRC-8 and --
 * through the linear CRC identity, without a pass over the payload -- CRC-16).  d_old is 16-byte aligned and unchanged; the
 * caller owns it, d_data, the workspace (fa_append_workspace_bytes[_i64]: the integer image, the encode's blob and its own
 * workspace) and d_bytes (fa_append_capacity_bytes[_i64] bytes: the old blob, the new encode's worst case and 6 bytes per new
 * frame; a smaller buffer gives FA_ERROR_ALLOC if the result does not fit, nothing outside it written).  The result is
 * d_bytes[0, *h_total_bytes), d_starts, d_nbytes [n_stream].  The call waits on `stream` for the tail decode and for the
 * total; the splice may still be queued when it returns: d_bytes / d_starts / d_nbytes are complete, and the workspace is
 * free again, when `stream` reaches the end of the call's work.  FA_ERROR_DECODE_INIT (before anything is decoded or
 * encoded): a stream without this encoder's SEEKTABLE, or whose STREAMINFO names another block size, channel count (1 for
 * the _i32 call, 2 for the _i64 call) or total sample count than stream_size. */
int64_t fa_append_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level);
int64_t fa_append_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level);
int64_t fa_append_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level);
int64_t fa_append_capacity_bytes_i64(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t n, uint32_t level);
int fa_append_i32_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                         int64_t n_stream, int64_t stream_size, const int32_t* d_data, int64_t n, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                         int64_t* h_total_bytes, void* stream);
int fa_append_i64_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                         int64_t n_stream, int64_t stream_size, const int64_t* d_data, int64_t n, uint32_t level, void* d_workspace,
                         int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes,
                         int64_t* h_total_bytes, void* stream);

/* Overwrite: replace samples [first, first + n) of m streams of a device-resident store (written by this library: one
 * SEEKTABLE point per frame) by d_data[m][n] -- int32 for one-channel streams (fa_overwrite_i32_device), int64 for
 * two-channel streams (fa_overwrite_i64_device) -- so that the result is, byte for byte, what fa_encode_i32_device /
 * fa_encode_i64_device writes for the patched samples (same level: its block size must be the one in the streams' STREAMINFO),
 * except that a stream which does not take part is copied whole, its STREAMINFO MD5 included, while a stream which takes part
 * gets a zero MD5.  d_stream_index[m]: the flat indices of the streams that take part, row j of d_data belonging to stream
 * d_stream_index[j]; NULL (with m == n_stream): all streams, in order.  With B the level's block size, F the frames per
 * stream, f0 = first / B and f1 = min(F, ceil((first + n) / B)): the span [f0 B, min(f1 B, stream_size)) of the m streams is
 * decoded (not when the range is the whole span), the new samples are laid over it, the (m, span) image is encoded, and one
 * splice kernel writes the result: per participating stream the header, the seek points and frames in front of the span
 * verbatim, the new frames renumbered k -> f0 + k (as fa_append_*_device renumbers), the frames behind the span verbatim and
 * their seek points with the offset moved.  Requires 0 <= first, n > 0, first + n <= stream_size
 * (FA_ERROR_DECODE_SAMPLE_RANGE) and 0 < m <= n_stream.  d_old is 16-byte aligned and unchanged; the caller owns it, d_data,
 * d_stream_index, the workspace (fa_overwrite_workspace_bytes[_i64]: the integer image, the encode's blob and its own
 * workspace) and d_bytes (fa_overwrite_capacity_bytes[_i64] bytes: the old blob, the span encode's worst case and 6 bytes per
 * new frame; a smaller buffer gives FA_ERROR_ALLOC if the result does not fit, nothing outside it written).  The result is
 * d_bytes[0, *h_total_bytes), d_starts, d_nbytes [n_stream].  The call waits on `stream` for the check, the span decode and
 * the total; the splice may still be queued when it returns: d_bytes / d_starts / d_nbytes are complete, and the workspace is
 * free again, when `stream` reaches the end of the call's work.  Before anything is decoded or encoded: FA_ERROR_DECODE_SEEK
 * for a stream index outside [0, n_stream) or named twice; FA_ERROR_DECODE_INIT for a participating stream without this
 * encoder's SEEKTABLE, whose STREAMINFO names another block size, channel count (1 for the _i32 call, 2 for the _i64 call)
 * or total sample count than stream_size, or whose seek offsets of frames f0 and f1 are not ordered inside its body. */
int64_t fa_overwrite_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level);
int64_t fa_overwrite_workspace_bytes_i64(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n, uint32_t level);
int64_t fa_overwrite_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n,
                                    uint32_t level);
int64_t fa_overwrite_capacity_bytes_i64(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t n,
                                        uint32_t level);
int fa_overwrite_i32_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                            int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const int32_t* d_data,
                            int64_t first, int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes,
                            int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream);
int fa_overwrite_i64_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                            int64_t n_stream, int64_t stream_size, const int64_t* d_stream_index, int64_t m, const int64_t* d_data,
                            int64_t first, int64_t n, uint32_t level, void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes,
                            int64_t capacity_bytes, int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream);

/* Quantisation with GIVEN per-stream offsets and gains (the inner loop of float32_to_int32 / float64_to_int64, utils.c:229-240
 * and :316-323, without the range pass): d_output[s * out_stride + i] for d_input[n_stream][n]; out_stride >= n lets the caller
 * write into a wider image.  What an append to a float store quantises its new samples with.  FA_ERROR_NAN_INPUT for a NaN
 * (the outputs are then unspecified).  Synchronises the stream. */
int fa_quantise_f32_device(const float* d_input, int64_t n_stream, int64_t n, const float* d_offsets, const float* d_gains, int32_t* d_output,
                           int64_t out_stride, void* stream);
int fa_quantise_f64_device(const double* d_input, int64_t n_stream, int64_t n, const double* d_offsets, const double* d_gains, int64_t* d_output,
                           int64_t out_stride, void* stream);

/* Decode [first_sample,last_sample) (or everything when either is negative) of n_stream
 * streams.  Exactly one of d_out_i32 / d_out_f32 is non-NULL; with d_out_f32 the int32 ->
 * float32 restore (utils.c:350-368) is fused into the store and d_offsets/d_gains[n_stream]
 * are required.  verify: see fa_set_decode_verify.  Returns the OR of the error bits (synchronises the stream).
 * Every decode entry point (this one, its two-channel twin, the slice calls and fa_decode_indexed) needs the output
 * pointer aligned to its element type only, takes arbitrary out_offset values as long as the slices' output ranges do
 * not overlap, and writes nothing outside the requested elements (tests/test_gpu_decode_footprint.py). */
int fa_decode_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                         const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t first_sample,
                         int64_t last_sample, int32_t* d_out_i32, float* d_out_f32, const float* d_offsets,
                         const float* d_gains, void* stream, int verify);

/* The same for two-channel (int64 / float64) streams; with d_out_f64 the int64 -> float64 restore
 * (int64_to_float64, utils.c:329-348) is fused into the final pass. */
int fa_decode_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                         const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t first_sample,
                         int64_t last_sample, int64_t* d_out_i64, double* d_out_f64, const double* d_offsets,
                         const double* d_gains, void* stream, int verify);

/* A decode index: the stream metadata and the byte offset of every frame of one store, computed once (K6) and kept in
 * device memory, for many reads of the same store -- the reference's usage pattern is one decode call per key
 * (array.py:409-449), and without an index every call parses every stream header again.  The store (d_bytes, 16-byte
 * aligned) must stay alive and unchanged while the index exists; channels = 1 (int32 / float32) or 2 (int64 / float64).
 * fa_decode_indexed: n_slices < 0 decodes [first_sample, last_sample) (or everything) of ALL streams, as
 * fa_decode_i32_device does; n_slices >= 0 is the batched random access of fa_decode_slices_i32_device.  d_out_int /
 * d_out_float are int32 / float32 for one channel, int64 / float64 for two (offsets / gains likewise). */
int fa_decode_index_create(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                           int64_t n_stream, int64_t stream_size, int channels, void** index, void* stream);
void fa_decode_index_destroy(void* index);
int fa_decode_indexed(void* index, int64_t first_sample, int64_t last_sample, int64_t n_slices, const int64_t* slice_stream,
                      const int64_t* slice_first, const int64_t* slice_count, const int64_t* out_offset, void* d_out_int,
                      void* d_out_float, const void* d_offsets, const void* d_gains, void* stream, int verify);

/* fa_decode_indexed for scattered slices whose samples are wanted on the HOST: the first out_bytes bytes of the result
 * are in h_out when the call returns.  For launches the latency decoder serves (up to 4096 frames) the kernel
 * writes them straight into host memory -- into h_out itself when that is pinned and device-visible (fa_pinned_alloc
 * below, or any hipHostMalloc), else into the library's own pinned landing buffer for results of up to 512 KB, copied
 * from there -- and the call synchronises once; otherwise the result is decoded into the caller's device buffer
 * (d_out_int / d_out_float as above, always required) and copied.  What the reference does for one small read:
 * seek_absolute + process_single into the caller's array, decompress.c:281-298. */
int fa_decode_indexed_host(void* index, int64_t n_slices, const int64_t* slice_stream, const int64_t* slice_first,
                           const int64_t* slice_count, const int64_t* out_offset, void* d_out_int, void* d_out_float,
                           const void* d_offsets, const void* d_gains, void* h_out, int64_t out_bytes, void* stream, int verify);

/* Pinned, device-visible host memory for results (hipHostMalloc / hipHostFree behind a C signature); NULL on failure.
 * flacarray_amd keeps a small pool of such blocks behind the numpy arrays its read paths return. */
void* fa_pinned_alloc(int64_t bytes);
void fa_pinned_free(void* p);

/* Integrity check of the decoder.  Every device decode entry point takes `verify`: 1 = re-compute the CRC-16 of each
 * frame the call read and report a mismatch as FA_ERROR_DECODE_PROCESS -- what libFLAC reports through the error
 * callback the reference prints (decompress.c:104-121) --, 0 = do not, negative = the process-wide default set here
 * (returns the previous setting; initially off).  The host-pointer decode_i32 / decode_i64 always check (libFLAC does;
 * FLACARRAY_HIP_HOST_VERIFY=0 turns that off).  The header CRC-8 of every frame is checked in all cases. */
int fa_set_decode_verify(int on);

/* Verification after encode, the counterpart of libFLAC's FLAC__stream_encoder_set_verify: when on, the host-pointer
 * encoders (encode_i32[_threaded], encode_i64[_threaded], fa_encode_f32_host, fa_encode_f64_host) decode every chunk of
 * streams they have just written, still on the device, and compare it with the chunk's input (float input as the
 * integers its offsets / gains quantise it to) before the input slot is released; a difference, or a stream the decoder
 * cannot read back, fails the call with FA_ERROR_ENCODE_VERIFY.  Process-wide; returns the previous setting (on < 0:
 * returns the setting and leaves it); initially off. */
int fa_set_encode_verify(int on);

/* ---- STREAMINFO MD5: the signature libFLAC writes into every stream (the MD5 of the samples it encodes, interleaved,
 * little-endian) and `flac -t` checks.  For the streams of this library -- 32 bits per sample, one channel (int32) or two
 * (int64: channel 0 = low word) -- the message is exactly the bytes of the integer row.  The encoders write sixteen zero
 * bytes ("not computed") unless signing is asked for; no encode, header or splice kernel knows about it: a signature is
 * computed by fa_md5_*_device and patched in by fa_sign_streams_device. ---- */

/* MD5 of every row of a device image, one lane per stream: d_data[s * row_stride + i], i < n, is int32 (fa_md5_i32_device)
 * or int64 (fa_md5_i64_device) -- or, when d_offsets / d_gains [n_stream] are given, float32 / float64 quantised with them
 * where it is loaded, exactly as the encoder quantises (FA_ERROR_NAN_INPUT for a NaN) -- so the signature of float input
 * is that of the integers any FLAC decoder will produce.  row_stride >= n (in elements) lets a column range of a wider
 * image be hashed.  Resumable: d_state[n_stream][4] is the per-stream chaining state, n_before the samples of every stream
 * hashed by earlier calls.  A call with final == 0 hashes a whole number of 64-byte blocks (n a multiple of 16 for int32 /
 * float32, of 8 for int64 / float64; FA_ERROR_CONVERT_TYPE otherwise) and writes d_state; the call with final != 0 (any n,
 * 0 included) hashes the padding and the bit length of all n_before + n samples and writes d_digest[n_stream][16].  d_state
 * is read only when n_before > 0 and may be NULL for a one-call hash; d_state and d_digest are 16-byte aligned.  Stream
 * order, no wait on the stream -- except for float input (one wait, for the NaN word). */
int fa_md5_i32_device(const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const float* d_offsets, const float* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, void* stream);
int fa_md5_i64_device(const void* d_data, int64_t n_stream, int64_t n, int64_t row_stride, const double* d_offsets, const double* d_gains,
                      uint32_t* d_state, int64_t n_before, int final, unsigned char* d_digest, void* stream);

/* Sign: write d_digests[s][16] into bytes [d_starts[s] + 26, d_starts[s] + 42) of d_bytes, the MD5 field of STREAMINFO.
 * Every stream must begin with "fLaC" and a STREAMINFO block inside d_bytes[0, n_bytes): FA_ERROR_DECODE_INIT otherwise,
 * and nothing is written.  Waits on the stream once (for that check); the patch itself is in stream order. */
int fa_sign_streams_device(unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, int64_t n_stream, const unsigned char* d_digests,
                           void* stream);

/* Check: decode the store (channels = 1: fa_decode_i32_device, 2: fa_decode_i64_device; `verify` and the error bits are
 * theirs) in column chunks of whole 64-byte blocks, each chunk hashed with the resumable kernel, and compare every stream's
 * digest with its STREAMINFO.  The decoded chunk -- the only large temporary -- stays under max_temp_bytes
 * (<= 0: FA_MD5_CHECK_TEMP_BYTES) unless one 64-byte block of every stream is more.  d_status[n_stream] (int8) receives
 * 1 = match, 0 = mismatch, -1 = unsigned (the field is all zero), -2 = not checkable: no STREAMINFO at the stream's start,
 * another channel count than `channels`, or not 32 bits per sample (libFLAC hashes those at ceil(bps / 8) bytes per sample;
 * this library decodes them to int32).  d_digests (may be NULL; 16-byte aligned) receives the computed digests [n_stream][16]
 * of the streams of status 1, 0 and -1.  A store without any stream to decide (and no digest asked for) is not decoded.
 * With more than one chunk the streams must share one block size, as every ranged decode needs.  Synchronises the stream. */
#define FA_MD5_CHECK_TEMP_BYTES (256LL << 20)
int fa_check_md5_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                        int64_t stream_size, int channels, int64_t max_temp_bytes, int8_t* d_status, unsigned char* d_digests, void* stream,
                        int verify);

/* Sign while encoding: when on, the host-pointer encoders (encode_i32[_threaded], encode_i64[_threaded], fa_encode_f32_host,
 * fa_encode_f64_host -- their argument lists are the reference's and cannot grow) hash every chunk of streams on the device
 * while its input is still there and patch the digests into the chunk's bytes before they go back to the host.
 * Process-wide; returns the previous setting (on < 0: returns the setting and leaves it); initially off, and with it off
 * every byte written is what it was before this entry point existed. */
int fa_set_encode_md5(int on);

/* Compare device-resident streams with the samples they should decode to, without writing the decoded samples anywhere:
 * d_first_mismatch[n_stream] (device) receives, per stream, the index of the first sample that differs, or -1.  What is
 * compared is integers: d_data is int32 for fa_compare_i32_device and int64 for fa_compare_i64_device, or -- when
 * d_offsets / d_gains [n_stream] are given -- float32 / float64 quantised with them exactly as the encoder does, so a
 * float change that leaves its quantised integer unchanged is not a difference.  Any stream the decoder reads is accepted
 * (streams without a SEEKTABLE are located by the sync scan).  A frame the decoder rejects, or cannot locate, marks its
 * stream at that frame's first sample or earlier and the other streams are still compared; only errors of the stream
 * headers (fLaC marker, STREAMINFO, stream size) are returned as the decoder's error bits, and so is a store whose streams
 * differ in block size (FA_ERROR_DECODE_INIT, as the decode entry points return it).  Device memory: the frame
 * table, and for two-channel streams the planar image fa_decode_i64_device uses too.  Synchronises the stream. */
int fa_compare_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                          int64_t n_stream, int64_t stream_size, const void* d_data, const float* d_offsets, const float* d_gains,
                          int64_t* d_first_mismatch, void* stream);
int fa_compare_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes,
                          int64_t n_stream, int64_t stream_size, const void* d_data, const double* d_offsets, const double* d_gains,
                          int64_t* d_first_mismatch, void* stream);

/* ---- Binned reduction: min, max, sum and sum of squares of the decoded integers, without a decoded copy.  Samples
 * [first, last) of every stream (both negative: the whole stream) are cut into nbins = ceil((last - first) / width) bins
 * [first + j * width, first + (j + 1) * width), the last one possibly short; a width beyond the range means one bin.  The
 * rows of the result are all n_stream streams (d_sel_streams NULL; n_sel is then ignored) or the n_sel streams that the
 * DEVICE array d_sel_streams names, in its order (an index outside [0, n_stream): FA_ERROR_DECODE_SAMPLE_RANGE; n_sel == 0
 * does nothing).  Outputs, device, [rows][nbins] in C order: d_min / d_max (int64, exact), d_sum (int64: exact for
 * one-channel streams, modulo 2^64 for two-channel ones, as a wrapping int64 sum is), and for one-channel streams
 * d_sq_hi / d_sq_lo (NULL together: not wanted), the two exact limbs of the sum of squares in radix 2^32: d_sq_lo = sum of
 * (x^2 mod 2^32), d_sq_hi = sum of (x^2 >> 32), sum of x^2 = d_sq_hi * 2^32 + d_sq_lo; exact below 2^32 samples per bin.
 * What is reduced is what any FLAC decoder produces -- for float stores the quantised integers.
 * One-channel streams are reduced inside the decoder (its store replaced by a sink that keeps each frame's running values
 * in registers: nothing but the bins is written); two-channel streams go through decoded column chunks of whole frames
 * that stay under max_temp_bytes (<= 0: FA_REDUCE_TEMP_BYTES; at least one frame of every row) -- a small cap saves memory
 * and costs time, since a chunk of few frames does not fill the decoder (profiles/reduce.md).  `verify`, the error bits and
 * the rule that all streams share one block size are the decode entry points'.  fa_reduce_indexed reduces the store of a
 * decode index (either channel count; d_sq_hi / d_sq_lo NULL, and max_temp_bytes used, for two channels only) without
 * parsing it again.  Everything is issued on `stream`, which is synchronised before returning. ---- */
#define FA_REDUCE_TEMP_BYTES (256LL << 20)
int fa_reduce_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                         int64_t stream_size, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams,
                         int64_t* d_min, int64_t* d_max, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify);
int fa_reduce_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                         int64_t stream_size, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams,
                         int64_t max_temp_bytes, int64_t* d_min, int64_t* d_max, int64_t* d_sum, void* stream, int verify);
int fa_reduce_indexed(void* index, int64_t first, int64_t last, int64_t width, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                      int64_t* d_min, int64_t* d_max, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify);

/* ---- fold across streams: per-sample sums over groups of streams, without a decoded copy.  Store, range [first, last)
 * (both negative: the whole stream), max_temp_bytes, `verify`, errors and stream ordering are fa_reduce_*'s.  The caller
 * hands in a plan of n = last - first columns, two DEVICE arrays of int64:
 *   d_order [n_sel]     the selected streams (no repeats), sorted by the group they belong to;
 *   d_rows [n_rows][3]  one row per 64 lanes of one group -- its group in [0, n_groups), the position in d_order of its
 *                       first stream, and how many of its 64 lanes are real (1..64); the rows of a group are adjacent
 *                       and together cover the group's streams once.  An empty group has no row.
 * An entry outside these bounds, or a stream outside [0, n_stream), is FA_ERROR_DECODE_SAMPLE_RANGE and is not added.
 * Outputs, device, [n_groups][n] in C order: d_sum (int64: the sum over the group's streams of sample first + j, exact for
 * one-channel streams, modulo 2^64 for two-channel ones) and for one-channel streams d_sq_hi / d_sq_lo (NULL together: not
 * wanted), the two exact limbs of the sum of squares in radix 2^32 as fa_reduce_* define them.  The call zero-fills the
 * outputs itself (the caller need not), but only after its arguments are accepted: a call refused with
 * FA_ERROR_CONVERT_TYPE, FA_ERROR_DECODE_SAMPLE_RANGE (an empty or misplaced range), FA_ERROR_ZERO_NSTREAM or
 * FA_ERROR_DECODE_STREAMSIZE has written nothing.  n_sel == 0 leaves zeros.
 * One-channel streams are summed inside the decoder: a wavefront decodes the same frame of the 64 streams of one plan row
 * and folds each column of its tile across its lanes, adding to the outputs with 64-bit atomics (integer adds commute:
 * the result does not depend on the order of arrival).  Two-channel streams go through decoded column chunks under
 * max_temp_bytes.  fa_xsum_indexed is the same on the store of a decode index (either channel count; d_sq_hi / d_sq_lo
 * NULL, and max_temp_bytes used, for two channels only).  Everything is issued on `stream`, which is synchronised before
 * returning. ---- */
int fa_xsum_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                       const int64_t* d_rows, int64_t n_groups, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify);
int fa_xsum_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                       int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                       const int64_t* d_rows, int64_t n_groups, int64_t max_temp_bytes, int64_t* d_sum, void* stream, int verify);
int fa_xsum_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows, const int64_t* d_rows,
                    int64_t n_groups, int64_t max_temp_bytes, int64_t* d_sum, uint64_t* d_sq_hi, uint64_t* d_sq_lo, void* stream, int verify);

/* ---- projections: exact inner products of the streams with K templates, without a decoded copy.  Store, range [first,
 * last) (both negative: the whole stream), max_temp_bytes, `verify`, errors and stream ordering are fa_reduce_*'s; the
 * selection comes as fa_xsum_*'s plan with ONE group, two DEVICE arrays of int64:
 *   d_order [n_sel]     the selected streams (no repeats), one result row each, in this order;
 *   d_rows [n_rows][3]  n_rows = ceil(n_sel / 64) rows [0, 64 * r, min(64, n_sel - 64 * r)].
 * An entry outside fa_xsum_*'s bounds, or a stream outside [0, n_stream), is FA_ERROR_DECODE_SAMPLE_RANGE and is not added;
 * no row beyond n_sel is ever written.
 * d_tmpl, device, is the template image, sample-major: int32 [n][ld] in C order with n = last - first, ld >= K, ld a
 * multiple of 8 and the padding columns zero; d_tmpl[j * ld + k] is template k at sample first + j.
 * Outputs, device, C order.  One-channel streams: d_hi (int64) and d_lo (uint64), [n_sel][K], the two radix-2^32 limbs of
 *     dot[r][k] = sum_j x[d_order[r]][first + j] * d_tmpl[j * ld + k] = d_hi * 2^32 + d_lo,
 * d_hi the sum of the products' upper words (p >> 32, arithmetic) and d_lo of their lower words: exact.  Two-channel
 * streams: d_out4 [n_sel][K][4], the limb pairs (hi, lo) of sum xl * t and of sum xh * t with x = xh * 2^32 + xl, xl
 * unsigned:  dot = ((out[2] * 2^32 + out[3]) * 2^32) + (out[0] * 2^32 + out[1]), out[0] and out[2] signed, out[1] and
 * out[3] unsigned: exact.
 * The call zero-fills the outputs itself (the caller need not), but only after its arguments are accepted: a call refused
 * with FA_ERROR_CONVERT_TYPE (a missing array, n_rows != ceil(n_sel / 64)), FA_ERROR_DECODE_SAMPLE_RANGE (an empty or
 * misplaced range, last - first > 2^32 - 1, K < 1, ld < K or ld not a multiple of 8), FA_ERROR_ZERO_NSTREAM or
 * FA_ERROR_DECODE_STREAMSIZE has written nothing.  n_sel == 0 writes nothing.
 * One-channel streams are multiplied inside the decoder: a wavefront decodes the same frame of 64 streams, so the template
 * values of a sample are the same for all its lanes and cost no per-lane memory traffic; 8 templates ride with one decode
 * of the range and K templates cost ceil(K / 8) decodes.  Lanes add their limbs with 64-bit atomics (integer adds commute:
 * the result does not depend on the order of arrival).  Two-channel streams go through decoded column chunks under
 * max_temp_bytes.  fa_dot_indexed is the same on the store of a decode index (d_hi / d_lo for one channel, d_out4 and
 * max_temp_bytes for two; the others may be NULL).  Everything is issued on `stream`, which is synchronised before
 * returning. ---- */
int fa_dot_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                      int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                      const int64_t* d_rows, int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t* d_hi, uint64_t* d_lo, void* stream, int verify);
int fa_dot_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                      int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows,
                      const int64_t* d_rows, int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t max_temp_bytes, int64_t* d_out4, void* stream,
                      int verify);
int fa_dot_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_order, int64_t n_rows, const int64_t* d_rows,
                   int64_t K, int64_t ld, const int32_t* d_tmpl, int64_t max_temp_bytes, int64_t* d_hi, uint64_t* d_lo, int64_t* d_out4,
                   void* stream, int verify);

/* ---- value histogram: counts per value bin of what the streams decode to, without a decoded copy.  Store, range, rows
 * (d_sel_streams / n_sel), max_temp_bytes, `verify`, errors and stream ordering are fa_reduce_*'s.  Every row r has its own
 * d_lo[r] (int64) and d_shift[r] (int32, 0..63), DEVICE arrays of `rows` elements; the call has one nbins, 1..2048
 * (otherwise FA_ERROR_CONVERT_TYPE).  A sample x of row r with x < d_lo[r] counts in d_below[r]; otherwise its bin is
 * b = ((uint64)x - (uint64)d_lo[r]) >> d_shift[r] (the unsigned difference is exact for every x >= lo), counted in
 * d_counts[r * nbins + b] when b < nbins and in d_above[r] otherwise: counts + below + above of a row is last - first.
 * Outputs are int64 device arrays, [rows][nbins] and [rows]; the call zeroes them on `stream` first.  One-channel streams
 * are counted inside the decoder (K7H: a per-wave histogram in LDS where the storing decoder keeps its tile image);
 * two-channel streams go through the decoded column chunks of fa_reduce_i64_device.  What is counted is what any FLAC
 * decoder produces -- for float stores the quantised integers (profiles/histogram.md). ---- */
int fa_histogram_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t nbins,
                            const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above, void* stream,
                            int verify);
int fa_histogram_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                            int64_t nbins, const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above,
                            void* stream, int verify);
int fa_histogram_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes, int64_t nbins,
                         const int64_t* d_lo, const int32_t* d_shift, int64_t* d_counts, int64_t* d_below, int64_t* d_above, void* stream, int verify);

/* ---- search: where are the samples outside per-row limits, without a decoded copy (profiles/find.md).  Store, range, rows
 * (d_sel_streams / n_sel), max_temp_bytes, `verify`, errors and stream ordering are fa_reduce_*'s.  d_lo / d_hi are int64
 * DEVICE arrays of `rows` elements; a sample x of row r is a hit iff (x < d_lo[r] || x > d_hi[r]) != (inside != 0) -- inside
 * == 0: outside the closed interval.  The search runs in two calls, with the caller's prefix sum between them:
 *   fa_find_plan_*   block_size and n_frames = the frames per row that meet [first, last) (host outputs).  The block size is
 *                    the index's, or the one stream 0's STREAMINFO states; a header that states none (minimum != maximum)
 *                    fails with FA_ERROR_DECODE_INIT.
 *   fa_find_count_*  d_frame_counts[row * n_frames + k] = hits in frame first / block_size + k of row `row` (int64 device
 *                    array of rows * n_frames elements, set to zero by the call on `stream` first).  n_frames must be the
 *                    number of frames the decoder works with: otherwise FA_ERROR_CONVERT_TYPE, and nothing is written.
 *   fa_find_fill_*   d_frame_offsets: rows * n_frames + 1 int64, the exclusive prefix sum of the counts (the last entry
 *                    the total); d_hit_tasks: the n_hit_tasks cells with a non-zero count, ascending.  Only those frames are
 *                    decoded again.  The k-th hit of cell c goes to d_pos[d_frame_offsets[c] + k] (the sample's index in its
 *                    stream) and, when d_val is not null, d_val[...] (its value, int64): hits come out sorted by (row,
 *                    position).  No cell writes more than its count.  Same limits, `inside`, range and rows as the count
 *                    call.  d_pos / d_val are complete only after the call's own synchronisation, i.e. when it returns.
 * No atomics place the hits: the result does not depend on the order of arrival.  One-channel streams are searched inside
 * the decoder (K7F); two-channel streams go through the decoded column chunks of fa_reduce_i64_device in BOTH calls.  What
 * is tested is what any FLAC decoder produces -- for float stores the quantised integers. ---- */
int fa_find_plan_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, int64_t stream_size, int64_t first, int64_t last,
                        int64_t* block_size, int64_t* n_frames, void* stream);
int fa_find_plan_indexed(void* index, int64_t first, int64_t last, int64_t* block_size, int64_t* n_frames);
int fa_find_count_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                             int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, const int64_t* d_lo,
                             const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream, int verify);
int fa_find_count_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                             int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                             const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream,
                             int verify);
int fa_find_count_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                          const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t* d_frame_counts, void* stream, int verify);
int fa_find_fill_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, const int64_t* d_lo,
                            const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                            const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify);
int fa_find_fill_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                            int64_t stream_size, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                            const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                            const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify);
int fa_find_fill_indexed(void* index, int64_t first, int64_t last, int64_t n_sel, const int64_t* d_sel_streams, int64_t max_temp_bytes,
                         const int64_t* d_lo, const int64_t* d_hi, int inside, int64_t n_frames, int64_t n_hit_tasks, const int64_t* d_hit_tasks,
                         const int64_t* d_frame_offsets, int64_t* d_pos, int64_t* d_val, void* stream, int verify);

/* ---- damage map and decode through errors.  The decode, compare, reduce and MD5 entry points give up a whole call for one
 * bad frame; these answer per (stream, frame), from nothing but the store, and decode what is intact.
 * fa_frame_status_device writes d_status[n_stream][nf] (device, one byte each), nf = ceil(stream_size / block_size):
 *   FA_FRAME_OK 0; FA_FRAME_UNLOCATED 1: the frame's extent is not known -- its stream is not wholly inside the blob, does
 *   not begin with "fLaC", its metadata chain does not parse inside nbytes, its STREAMINFO does not say min == max block
 *   size == block_size with `channels` channels (1: int32 / float32 arrays, 2: int64 / float64), it has no SEEKTABLE of
 *   exactly nf points, or seek point f or f + 1 does not carry its own sample number or gives an extent that is not at
 *   least 8 bytes inside the stream (a bad seek point k therefore marks frames k - 1 and k; streams without a per-frame
 *   SEEKTABLE, such as libFLAC's, are UNLOCATED throughout); for located frames the two independent bits
 *   FA_FRAME_HEADER 2: the frame header is one the decoder rejects (sync / reserved bits, block-size, sample-rate,
 *   sample-size or channel code, CRC-8), its number is not f, or its block size is not min(block_size, stream_size - f *
 *   block_size); FA_FRAME_CRC16 4: the CRC-16 of the frame's bytes is not the stored one.
 * A frame is decodable exactly when its status is 0.  The check is as strong as CRC-16: a random change escapes it with
 * probability 2^-16 (fa_check_md5_device is the stronger check, per stream).  However damaged the store is the return
 * code is FA_ERROR_NONE: non-zero means bad arguments (n_stream <= 0, stream_size <= 0, block_size outside 1..65535,
 * channels not 1 or 2, a null pointer) or a HIP failure.  No byte is read before its offset is checked against the blob.
 * fa_fill_ranges_device writes the element at fill_value (host, elem_bytes = 4 or 8 bytes) over n_ranges ranges of d_out:
 * elements [d_off[i], d_off[i] + d_count[i]) (device arrays; any alignment); nothing else is written; not waited for.
 * fa_decode_salvage_i32_device / _i64_device take the arguments of fa_decode_i32_device / fa_decode_i64_device (the range,
 * an integer or a float output, offsets and gains) and block_size, fill_value (host; one output element) and d_status: the
 * status pass runs over the whole store and lands in d_status, every frame of status 0 that touches the range is decoded
 * exactly (frame CRC-16 check off: it has just been made), and the samples of every other frame are fill_value.  An error
 * the decoder still reports (a CRC-clean frame beyond its subset) is returned as by fa_decode_*_device.
 * All work is issued on `stream`; the status and salvage calls synchronise it before returning. ---- */
#define FA_FRAME_OK 0
#define FA_FRAME_UNLOCATED 1
#define FA_FRAME_HEADER 2
#define FA_FRAME_CRC16 4
int fa_frame_status_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                           int64_t stream_size, int channels, int64_t block_size, unsigned char* d_status, void* stream);
int fa_fill_ranges_device(void* d_out, int elem_bytes, int64_t n_ranges, const int64_t* d_off, const int64_t* d_count, const void* fill_value,
                          void* stream);
int fa_decode_salvage_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                                 int64_t stream_size, int64_t first_sample, int64_t last_sample, int32_t* d_out_i32, float* d_out_f32,
                                 const float* d_offsets, const float* d_gains, int64_t block_size, const void* fill_value, unsigned char* d_status,
                                 void* stream);
int fa_decode_salvage_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts, const int64_t* d_nbytes, int64_t n_stream,
                                 int64_t stream_size, int64_t first_sample, int64_t last_sample, int64_t* d_out_i64, double* d_out_f64,
                                 const double* d_offsets, const double* d_gains, int64_t block_size, const void* fill_value, unsigned char* d_status,
                                 void* stream);

/* Reindex: copy every stream of a store into this library's own layout -- "fLaC", STREAMINFO (the source's 34 bytes
 * verbatim, MD5 included, marked not last), a SEEKTABLE of one point per frame (sample number f B, offset of frame f from
 * the first frame, min(B, N - f B) samples), then the source's frames [first frame, end of stream) verbatim.  No sample is
 * decoded and nothing is re-encoded; every other metadata block of the source (VORBIS_COMMENT, APPLICATION, PADDING, a
 * sparse or placeholder SEEKTABLE) is dropped; a stream that already has the layout comes out byte-identical.  This is how
 * a libFLAC-written store, which the decoders read but append, overwrite and the damage map refuse, becomes a store of
 * this library.  The frames are located as the decoders locate them (a complete SEEKTABLE, else the sync scan, else the
 * walk), so one call takes streams of ONE block size and n_channels (1: int32 / float32 arrays, 2: int64 / float64), and
 * the decoders' errors come back as they are: FA_ERROR_DECODE_INIT for a stream header that does not parse, a variable
 * block size, streams that differ in block size, or the other channel count; FA_ERROR_DECODE_PROCESS for a walk that
 * leaves its stream.  On top of that the frame table must start at the first frame, increase strictly and leave 8 bytes
 * for the last frame inside its stream (FA_ERROR_DECODE_SEEK otherwise: the offsets of a SEEKTABLE are the file's word,
 * and the copy would follow them), the last frame located must carry frame number nf - 1 and the block size that
 * stream_size leaves for it (FA_ERROR_DECODE_STREAMSIZE: the stream_size is not the store's), the first metadata block
 * must be a STREAMINFO of 34 bytes, and a stream has at most 932 067 frames, what the SEEKTABLE's 24-bit length holds
 * (FA_ERROR_DECODE_INIT).  d_old may have any alignment (a
 * misaligned blob is realigned through the library's scratch) and is unchanged; d_bytes must not overlap it and has room
 * for capacity_bytes; fa_reindex_capacity_bytes() = n_old_bytes + n_stream * (46 + 18 nf) always suffices (-1 for
 * arguments that make no store), a smaller buffer gives FA_ERROR_ALLOC if the result does not fit.  On every error
 * nothing is written to d_bytes.  The new streams lie back to back from 0 in the old order, d_starts / d_nbytes
 * [n_stream] are their index, *h_total_bytes the bytes used.  n_stream == 0 returns FA_ERROR_NONE with a total of 0 and
 * launches nothing.  All device work is issued on `stream`, which the call waits for before it returns; the frame tables
 * are allocated and freed per call as fa_decode_index_create / _destroy do, and those two runtime calls wait for the whole
 * device, not for `stream` alone.  Because the last frame's header ties stream_size to the store, a store whose damage
 * sits in the header of a stream's LAST frame is refused (FA_ERROR_DECODE_STREAMSIZE) like a wrong stream_size. */
int64_t fa_reindex_capacity_bytes(int64_t n_old_bytes, int64_t n_stream, int64_t stream_size, int64_t block_size);
int fa_reindex_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes,
                      int64_t n_stream, int64_t stream_size, int n_channels, unsigned char* d_bytes, int64_t capacity_bytes,
                      int64_t* d_starts, int64_t* d_nbytes, int64_t* h_total_bytes, void* stream);

/* Window: cut samples [first, last) of m streams of a store out as a NEW store of m streams, without re-encoding the
 * frames that are kept whole (window_kernels.hpp, K14).  `first` must be a multiple of the block size B of `level`
 * (FA_ERROR_DECODE_SAMPLE_RANGE otherwise, as for first < 0, last > stream_size and last <= first: with an unaligned
 * first every frame boundary moves and the window has to be decoded and encoded, which is the caller's to do).  The
 * frames f0 = first / B, f0 + 1, ... are copied with their numbers lowered by f0 (the UTF-8 number field, the header
 * CRC-8, and the CRC-16 through its linear identity: no pass over a payload), the seek table is rebuilt in closed form
 * from the old one, and the stream header is written for last - first samples with a zero MD5.  Where last falls inside
 * an old frame (and is not the old end) that one frame is decoded up to the cut and encoded again as a short last
 * frame; where last == stream_size the old last frame is one more kept frame.  For integer stores the result is byte
 * for byte the encode of the decoded window at `level`, provided that is the level the store was written at.  Two
 * shortcuts: first == 0 renumbers nothing (the kept points and frames are copied as they are); first == 0 && last ==
 * stream_size copies every picked stream verbatim, its STREAMINFO MD5 included (pure stream selection).
 * d_stream_index: m flat stream indices (device), the output order; NULL: all streams (m == n_stream).  An index out of
 * range or named twice gives FA_ERROR_ZERO_NSTREAM.  m == 0 returns FA_ERROR_NONE with a total of 0 and launches nothing.
 * channels: 1 for int32 / float32 arrays, 2 for int64 / float64 (no sample format enters the copy; the tail decode and
 * encode pick their path from it).  Every picked stream must be one this library wrote for the call's block size,
 * channel count and stream size, with one seek point per frame (FA_ERROR_DECODE_INIT otherwise; fa_reindex_device
 * adopts other stores), and every seek offset of the frames the call follows must be ordered inside the stream's body
 * and leave each frame its own header plus the CRC-16, at least 13 bytes (FA_ERROR_DECODE_SEEK otherwise).  Both are
 * checked by one kernel before anything is decoded or copied, and on every error nothing is written to d_bytes.
 * d_old and d_workspace must be 16-byte aligned (FA_ERROR_ENCODE_INIT); d_old is unchanged and d_bytes must not overlap
 * it.  fa_window_workspace_bytes() is the workspace the call needs; fa_window_capacity_bytes(n_picked_bytes, ...) a
 * capacity that always suffices, given the bytes of the picked streams or any upper bound of them (the whole old blob,
 * say): a kept frame never grows, so the bound is those bytes plus the worst case of the re-encoded frame; a smaller
 * buffer gives FA_ERROR_ALLOC if the result does not fit.  Both return -1 for arguments the call refuses.  The new
 * streams lie back to back from 0 in the order asked, d_starts / d_nbytes [m] are their index, *h_total_bytes the bytes
 * used; no byte of d_bytes from there on is written.  All work is issued on `stream`; the copy is not waited for. */
int64_t fa_window_workspace_bytes(int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t last, int channels, uint32_t level);
int64_t fa_window_capacity_bytes(int64_t n_picked_bytes, int64_t n_stream, int64_t stream_size, int64_t m, int64_t first, int64_t last,
                                 int channels, uint32_t level);
int fa_window_device(const unsigned char* d_old, int64_t n_old_bytes, const int64_t* d_old_starts, const int64_t* d_old_nbytes, int64_t n_stream,
                     int64_t stream_size, const int64_t* d_stream_index, int64_t m, int64_t first, int64_t last, int channels, uint32_t level,
                     void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                     int64_t* d_nbytes, int64_t* h_total_bytes, void* stream);

/* Join: put the streams of n_parts stores of n_stream streams each behind one another along the sample axis as a NEW
 * store, without decoding a sample or re-encoding a frame (join_kernels.hpp, K15; the inverse of the window).  Part p
 * holds stream_sizes[p] samples per stream; every part but the last must be a whole number of blocks B of `level` long
 * (FA_ERROR_DECODE_SAMPLE_RANGE otherwise: every frame boundary behind an unaligned part moves, and the decode and encode
 * that takes is the caller's to do; the same code for a total of 2^36 samples or more).  With base_p the frames in front
 * of part p, frame k of part p is copied as frame base_p + k (the UTF-8 number field, which may get longer, the header
 * CRC-8, and the CRC-16 through its linear identity: no pass over a payload), the seek table is rebuilt in closed form
 * from the parts' tables, and the stream header is written for the total samples with a zero MD5.  For integer stores
 * the result is byte for byte the encode of the concatenated decoded parts at `level`, provided that is the level every
 * part was written at.  Two shortcuts: part 0 changes neither numbers nor offsets, its seek points and frames are copied
 * as they are; n_parts == 1 copies every stream verbatim, its STREAMINFO MD5 included.
 * d_old, n_old_bytes, d_old_starts, d_old_nbytes and stream_sizes are HOST arrays of length n_parts (of device pointers,
 * byte counts and sizes); the part descriptors travel to the device in the workspace, so n_parts is bounded by the
 * implementation only: at most 65536 (FA_ERROR_ENCODE_PROCESS, as for more than 932 067 frames per stream, what the
 * SEEKTABLE's 24-bit length holds).  n_parts <= 0 gives FA_ERROR_ZERO_NSTREAM, a stream size <= 0 FA_ERROR_ZERO_STREAMSIZE;
 * n_stream == 0 returns FA_ERROR_NONE with a total of 0 and launches nothing.  channels: 1 for int32 / float32 arrays,
 * 2 for int64 / float64 (no sample format enters the copy).  Every stream of every part must be one this library wrote
 * for the call's block size, channel count and that part's stream size, with one seek point per frame
 * (FA_ERROR_DECODE_INIT otherwise; fa_reindex_device adopts other stores), and every seek offset of every part must be
 * ordered inside the stream's body and leave each frame its own header plus the CRC-16, at least 13 bytes
 * (FA_ERROR_DECODE_SEEK otherwise).  Both are checked by one kernel before anything is copied, and on every error nothing
 * is written to d_bytes.  Every d_old[p] and d_workspace must be 16-byte aligned (FA_ERROR_ENCODE_INIT); the parts are
 * unchanged, may be one and the same store, and d_bytes must not overlap them.  fa_join_workspace_bytes() is the
 * workspace the call needs; fa_join_capacity_bytes() a capacity that always suffices: the parts' bytes plus
 * n_stream * (46 + the growth of the number fields), since the seek points only move; a smaller buffer gives
 * FA_ERROR_ALLOC if the result does not fit.  Both return -1 for arguments the call refuses.  The new streams lie back to
 * back from 0, d_starts / d_nbytes [n_stream] are their index, *h_total_bytes the bytes used; no byte of d_bytes from
 * there on is written.  All work is issued on `stream`; the copy is not waited for, and reads the workspace. */
int64_t fa_join_workspace_bytes(int64_t n_parts, int64_t n_stream, const int64_t* stream_sizes, int channels, uint32_t level);
int64_t fa_join_capacity_bytes(int64_t n_parts, const int64_t* n_old_bytes, int64_t n_stream, const int64_t* stream_sizes, int channels,
                               uint32_t level);
int fa_join_device(int64_t n_parts, const unsigned char* const* d_old, const int64_t* n_old_bytes, const int64_t* const* d_old_starts,
                   const int64_t* const* d_old_nbytes, const int64_t* stream_sizes, int64_t n_stream, int channels, uint32_t level,
                   void* d_workspace, int64_t workspace_bytes, unsigned char* d_bytes, int64_t capacity_bytes, int64_t* d_starts,
                   int64_t* d_nbytes, int64_t* h_total_bytes, void* stream);

/* Batched random access: slice i is samples [first[i], first[i]+count[i]) of stream
 * slice_stream[i]; its samples are written at element offset out_offset[i] of the output.
 * The four slice arrays are HOST arrays of length n_slices.  The reference needs one
 * decode_i32 call per slice for this (decompress.py:42-48: one range for all streams). */
int fa_decode_slices_i32_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                                const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t n_slices,
                                const int64_t* slice_stream, const int64_t* slice_first, const int64_t* slice_count,
                                const int64_t* out_offset, int32_t* d_out_i32, float* d_out_f32,
                                const float* d_offsets, const float* d_gains, void* stream, int verify);

int fa_decode_slices_i64_device(const unsigned char* d_bytes, int64_t n_bytes, const int64_t* d_starts,
                                const int64_t* d_nbytes, int64_t n_stream, int64_t stream_size, int64_t n_slices,
                                const int64_t* slice_stream, const int64_t* slice_first, const int64_t* slice_count,
                                const int64_t* out_offset, int64_t* d_out_i64, double* d_out_f64,
                                const double* d_offsets, const double* d_gains, void* stream, int verify);

/* float32 -> int32 quantisation on device; d_quanta may be NULL.  Returns FA_ERROR_NAN_INPUT
 * if any input is NaN (outputs are then unspecified).  The four conversions of this group launch one workgroup per
 * stream (to integers) or per 16384-sample chunk of a stream (to floats): more than 2^31 - 1 of them are refused with
 * FA_ERROR_CONVERT_TYPE before anything is launched or touched (convert the streams in groups). */
int fa_float32_to_int32_device(const float* d_input, int64_t n_stream, int64_t stream_size, const float* d_quanta,
                               int32_t* d_output, float* d_offsets, float* d_gains, void* stream);

int fa_int32_to_float32_device(const int32_t* d_input, int64_t n_stream, int64_t stream_size, const float* d_offsets,
                               const float* d_gains, float* d_output, void* stream);

/* The float64 <-> int64 twins (utils.c:245-348) on device pointers. */
int fa_float64_to_int64_device(const double* d_input, int64_t n_stream, int64_t stream_size, const double* d_quanta,
                               int64_t* d_output, double* d_offsets, double* d_gains, void* stream);
int fa_int64_to_float64_device(const int64_t* d_input, int64_t n_stream, int64_t stream_size, const double* d_offsets,
                               const double* d_gains, double* d_output, void* stream);

/* Per-stream standard deviation of d_in[n_stream][stream_size] (C-contiguous, device) into d_out[n_stream], bit for bit
 * what numpy's np.std(x, axis=-1) gives for the contiguous host copy when np.getbufsize() == chunk: each row is summed
 * in chunks of `chunk` elements (numpy's pairwise sum per chunk, chunk sums added in order), mean = T(double(sum) / n),
 * then the same sum of T((x - mean)^2), var = T(double(sum) / n), std = sqrt(var) correctly rounded; a NaN gives NaN.
 * Four launches in stream order, no wait on the stream -- except once when (stream_size, chunk) changes and the chunk
 * needs a summation plan (any chunk length other than 8192; flacarray_amd/npsum.py pairwise_plan): the plan is uploaded.
 * Workspace: the library's per-device scratch (n_stream * ceil(stream_size / chunk) + n_stream values), so calls of one
 * device on different streams must not overlap.  FA_ERROR_CONVERT_TYPE for chunk <= 0 or more than 2^31 - 1 chunks. */
int fa_stream_std_f32_device(const float* d_in, int64_t n_stream, int64_t stream_size, int64_t chunk, float* d_out, void* stream);
int fa_stream_std_f64_device(const double* d_in, int64_t n_stream, int64_t stream_size, int64_t chunk, double* d_out, void* stream);

/* Kernel timing for bench.py: when enabled, HIP events are recorded on the launch stream around
 * the three dominant kernels of the most recent calls; fa_profile_last waits for them and
 * returns milliseconds {encode_frames_kernel, compact_frames_kernel, decode_frames_kernel<8>}
 * (-1 for a kernel that has not run). */
void fa_profile_enable(int on);
int fa_profile_last(float* ms3);
/* The same with more pairs: ms[0..n) = {encode_frames_kernel, compact_frames_kernel, decode_frames_kernel<8>,
 * whole encode sequence (first launch of _begin .. last launch of _finish, host gaps included),
 * whole decode sequence (K6 + K7), float32_to_int32_kernel}; n <= 6. */
int fa_profile_read(float* ms, int n);

/* free the library's cached device scratch (decode tables, staging buffers) */
void fa_release_scratch(void);

/* Diagnostic, for the test suite only (no library code, tool or benchmark calls them).
 * fa_debug_scratch_fill(byte), byte in 0..255: waits for the device, fills every cached scratch slot over its whole
 * allocation with `byte`, drops what the library caches inside slots (the encoders' frame-header table, the std
 * summation plans), and from then on fills every slot it allocates with `byte` as well.  byte = -1 turns that sticky fill
 * off again (the default).  FA_ERROR_ALLOC for any other value.
 * fa_debug_scratch_bytes(out, n): out[i] = the bytes slot i holds now, i < min(n, slots); returns the number of slots. */
int fa_debug_scratch_fill(int byte);
int fa_debug_scratch_bytes(int64_t* out, int n);

/* number of visible HIP devices (0 when there is no GPU); never initialises a context */
int fa_device_count(void);

/* library version string */
const char* fa_version(void);

/* ABI revision of the group-2 (fa_*) signatures in this header.  It is raised whenever an existing entry point changes
 * its argument list (revision 2: the trailing `int verify` of the device decode entry points, 1 / 0 / negative = check /
 * do not / process default, see fa_set_decode_verify; revision 3 added the std entry points, revision 4 the compare entry
 * points and fa_set_encode_verify); a binding built against
 * another revision must refuse the library instead of calling it with a shifted argument list --
 * flacarray_amd/_lib.py does.  Entry points that are only added (the append, MD5, overwrite, damage-map, reindex, window and join groups) leave it as it is. */
#define FA_ABI_VERSION 4  /* (revision 4: fa_compare_i32_device / fa_compare_i64_device / fa_set_encode_verify) */
int fa_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLACARRAY_HIP_H */
