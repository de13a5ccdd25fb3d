"""Host side of the damage map: the status constants, the block size a store was written with, and the sample ranges a
status array fences off.  Pure numpy: nothing here loads the library or touches a GPU.

The status of a (stream, frame) is 0 (FRAME_OK: decodable), FRAME_UNLOCATED (its extent is not known: the stream header,
the SEEKTABLE or a seek point of the frame or of its successor is bad), or a combination of FRAME_HEADER (the frame
header, its frame number or its block size is wrong) and FRAME_CRC16 (the frame's CRC-16 is wrong).  The check is as
strong as CRC-16: a random change escapes it with probability 2^-16; `check_md5` is the stronger check, per stream."""
import numpy as np

FRAME_OK = 0
FRAME_UNLOCATED = 1
FRAME_HEADER = 2
FRAME_CRC16 = 4


def common_block_size(header_bytes):
    """The most common STREAMINFO block size (the smallest of them on a tie) among streams given by their first 12
    bytes (uint8 [k, 12]: "fLaC", the STREAMINFO block header, min and max block size), counting streams whose two
    block sizes agree and are not zero; None when there is no such stream."""
    h = np.asarray(header_bytes, dtype=np.uint8).reshape(-1, 12)
    bmin = (h[:, 8].astype(np.int64) << 8) | h[:, 9]
    bmax = (h[:, 10].astype(np.int64) << 8) | h[:, 11]
    sizes = bmax[(bmin == bmax) & (bmax > 0)]
    if sizes.size == 0:
        return None
    values, counts = np.unique(sizes, return_counts=True)
    return int(values[np.argmax(counts)])  # (np.unique sorts: argmax takes the smallest of equally common sizes)


def readable_streams(starts, nbytes, blob_bytes):
    """Mask of the streams whose first 12 bytes lie inside their extent and inside the blob."""
    st, nb = np.asarray(starts, dtype=np.int64).reshape(-1), np.asarray(nbytes, dtype=np.int64).reshape(-1)
    return (st >= 0) & (nb >= 12) & (st <= blob_bytes - 12)


def store_block_size(blob, starts, nbytes):
    """common_block_size over a host store; raises when no stream header can be read."""
    blob = np.asarray(blob, dtype=np.uint8).reshape(-1)
    st = np.asarray(starts, dtype=np.int64).reshape(-1)
    st = st[readable_streams(st, nbytes, blob.size)]
    b = common_block_size(blob[st[:, None] + np.arange(12)[None, :]]) if st.size else None
    if b is None:
        raise RuntimeError("No stream header gives a block size: pass block_size")
    return b


def damaged_ranges(status, block_size, stream_size):
    """The sample ranges of the frames whose status is not 0: int64 [k, 3], rows (flat stream, first, last) with `last`
    exclusive, adjacent frames of a stream merged, sorted by (stream, first).  `status`: leading shape + (nf,)."""
    st = np.asarray(status)
    nf = -(-int(stream_size) // int(block_size))
    if st.shape[-1:] != (nf,):
        raise ValueError(f"status has {st.shape[-1:]} frames per stream, {nf} expected")
    bad = (st.reshape(-1, nf) != 0).astype(np.int8)
    edge = np.diff(np.pad(bad, ((0, 0), (1, 1))), axis=1)  # +1 where a run of damaged frames begins, -1 behind its end
    rows, begin = np.nonzero(edge == 1)
    _, end = np.nonzero(edge == -1)
    out = np.empty((rows.size, 3), dtype=np.int64)
    out[:, 0] = rows
    out[:, 1] = begin * int(block_size)
    out[:, 2] = np.minimum(end * int(block_size), int(stream_size))
    return out
