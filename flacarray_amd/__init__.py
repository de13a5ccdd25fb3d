"""flacarray_amd -- MI355X-native FLAC encode/decode path behind flacarray's operator API.

Drop-in names of the reference (hpc4cmb/flacarray): `array_compress`, `array_decompress`,
`array_decompress_slice`, `encode_flac`, `decode_flac`, `float_to_int`, `int_to_float`,
`FlacArray`.  `array_encode` / `array_decode` are aliases for the spelling used in
BASELINE.json.  All compute runs in hand-written HIP kernels (libflacarray_hip.so); there is
no CPU fallback.
"""
from .array import CrossStreamStats, FlacArray, StreamHistogram, StreamHits, StreamStats
from .compress import array_compress
from .decompress import array_decompress, array_decompress_slice
from .libflacarray import (
    DeviceDecodeIndex,
    append_flac_device,
    check_md5_device,
    compare_flac_device,
    decode_flac,
    decode_flac_device,
    decode_flac_salvage_device,
    decode_slices_device,
    encode_flac,
    encode_flac_device,
    encode_flac_device_f32,
    encode_flac_device_f64,
    float32_to_int32_device,
    float64_to_int64_device,
    frame_status_device,
    join_flac_device,
    md5_device,
    overwrite_flac_device,
    reduce_flac_device,
    common_mode_flac_device,
    histogram_flac_device,
    find_flac_device,
    find_counts_flac_device,
    reindex_flac_device,
    set_decode_verify,
    set_encode_md5,
    set_encode_verify,
    sign_streams_device,
    std_device,
    window_flac_device,
)
from .scrub import FRAME_CRC16, FRAME_HEADER, FRAME_OK, FRAME_UNLOCATED, damaged_ranges
from .utils import float_to_int, int_to_float, keep_select, stream_md5

array_encode = array_compress
array_decode = array_decompress

__version__ = "0.1.0"

__all__ = [
    "FlacArray",
    "StreamHistogram",
    "StreamHits",
    "StreamStats",
    "CrossStreamStats",
    "DeviceDecodeIndex",
    "append_flac_device",
    "overwrite_flac_device",
    "reindex_flac_device",
    "window_flac_device",
    "join_flac_device",
    "array_compress",
    "array_decompress",
    "array_decompress_slice",
    "array_encode",
    "array_decode",
    "encode_flac",
    "decode_flac",
    "encode_flac_device",
    "encode_flac_device_f32",
    "encode_flac_device_f64",
    "decode_flac_device",
    "decode_slices_device",
    "frame_status_device",
    "decode_flac_salvage_device",
    "damaged_ranges",
    "FRAME_OK",
    "FRAME_UNLOCATED",
    "FRAME_HEADER",
    "FRAME_CRC16",
    "compare_flac_device",
    "reduce_flac_device",
    "common_mode_flac_device",
    "histogram_flac_device",
    "find_flac_device",
    "find_counts_flac_device",
    "md5_device",
    "check_md5_device",
    "sign_streams_device",
    "stream_md5",
    "set_encode_md5",
    "float32_to_int32_device",
    "float64_to_int64_device",
    "std_device",
    "set_decode_verify",
    "set_encode_verify",
    "float_to_int",
    "int_to_float",
    "keep_select",
]
