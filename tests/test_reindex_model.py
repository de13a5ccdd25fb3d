"""Preconditions of the reindex tests, on the CPU: tests/reindex_model.py turns every foreign layout of the stream writer
into the writer's own-layout twin byte for byte, its outputs decode to the writer's samples and are intact by the damage
map's rule, and to_foreign followed by the model is the identity on stores the CPU encoder wrote.
tests/test_gpu_reindex.py compares the GPU with the same model."""
import numpy as np
import pytest

from tests import reindex_model as R
from tests import scrub_model as SM
from tests.golden import flac_writer as W

FOREIGN = ("libflac", "placeholder", "sparse", "padded")
# (channels, block, samples): a short last frame everywhere; 25 frames reach the sparse table's third point
GEOMETRIES = ((1, 192, 24 * 192 + 77), (2, 64, 11 * 64 + 5))


def _twins(seed, channels, block, n, layout):
    """write_stream twice from a fresh generator, identical but for the layout."""
    a = W.write_stream(np.random.default_rng(seed), n, block, channels, layout=layout)
    b = W.write_stream(np.random.default_rng(seed), n, block, channels, layout="own")
    return a, b


@pytest.fixture(scope="module")
def twins():
    out = {}
    for g, (channels, block, n) in enumerate(GEOMETRIES):
        for k, layout in enumerate(FOREIGN):
            out[(channels, layout)] = _twins(1000 + 10 * g + k, channels, block, n, layout) + ((channels, block, n),)
    return out


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("layout", FOREIGN)
def test_twins(twins, oracle, channels, layout):
    (x, foreign, rec), (x_own, own, _), (_, block, n) = twins[(channels, layout)]
    assert n % block and rec["layout"] == layout
    # the same samples and the same frames
    assert np.array_equal(x, x_own)
    assert foreign[R.first_frame(foreign) :] == own[R.first_frame(own) :]
    assert foreign != own and foreign[8:42] == own[8:42]
    offs = R.find_frames(foreign, n, block, channels)
    assert [o - offs[0] for o in offs] == [o - R.own_offsets(own)[0] for o in R.own_offsets(own)]
    model = R.reindex_stream(foreign, offs, n, block)
    assert model == own
    # the model of the own twin is the identity
    assert R.find_frames(own, n, block, channels) == R.own_offsets(own)
    assert R.reindex_stream(own, R.own_offsets(own), n, block) == own
    # the oracle decodes the model output to the writer's samples
    blob, st, nb = W.pack([model])
    dec = oracle.decode_i32 if channels == 1 else oracle.decode_i64
    assert np.array_equal(dec(blob, st, nb, n)[0], x)
    # intact by the damage map's rule; the libFLAC layout is nowhere located
    assert not SM.frame_status(blob, st, nb, n, channels, block).any()
    if layout == "libflac":
        fb, fst, fnb = W.pack([foreign])
        assert (SM.frame_status(fb, fst, fnb, n, channels, block) == SM.UNLOCATED).all()


def test_store_model_packs_back_to_back(twins):
    (_, f1, _), (_, o1, _), (channels, block, n) = twins[(1, "libflac")]
    (_, f2, _), (_, o2, _), _ = twins[(1, "padded")]
    junk = b"\xa5" * 7
    blob = np.frombuffer(junk + f1 + junk + f2, dtype=np.uint8)
    st = np.array([7, 14 + len(f1)], dtype=np.int64)
    nb = np.array([len(f1), len(f2)], dtype=np.int64)
    got = R.reindex_store(blob, st, nb, n, block, channels)
    want = W.pack([o1, o2])
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("wide", (False, True))
def test_to_foreign_then_the_model_is_the_identity(oracle, wide):
    from tests.conftest import full_range_i32
    from tests.verify_corpus import full_range_i64

    n, block = 2 * 1152 + 300, 1152
    if wide:
        data = full_range_i64((3, n), seed=31)
        blob, st, nb = oracle.encode_i64(data, 1)
    else:
        data = full_range_i32((3, n), seed=30)
        blob, st, nb = oracle.encode_i32(data, 1)
    nch = 2 if wide else 1
    fb, fst, fnb = R.to_foreign(blob, st, nb)
    assert fb.size == blob.size + 3 * (len(W._vorbis()) - 18 * 3)
    assert (SM.frame_status(fb, fst, fnb, n, nch, block) == SM.UNLOCATED).all()
    dec = oracle.decode_i64 if wide else oracle.decode_i32
    assert np.array_equal(dec(fb, fst, fnb, n), data)
    back = R.reindex_store(fb, fst, fnb, n, block, nch)
    assert np.array_equal(back[0], blob) and np.array_equal(back[1], st) and np.array_equal(back[2], nb)


def test_host_interface(oracle):
    """The names exist, and has_frame_index reads the layout from the host copy alone (no device is touched)."""
    import flacarray_amd as fa
    from flacarray_amd import _lib
    from tests.conftest import full_range_i32

    assert "reindex_flac_device" in fa.__all__ and callable(fa.reindex_flac_device)
    assert {"fa_reindex_capacity_bytes", "fa_reindex_device"} <= set(_lib.SYMBOLS)
    n = 4096 + 100
    data = full_range_i32((2, 2, n), seed=32)
    blob, st, nb = oracle.encode_i32(data.reshape(4, n), 5)
    make = lambda t: fa.FlacArray(None, shape=data.shape, compressed=t[0], dtype=np.int32, stream_starts=t[1].reshape(2, 2),  # noqa: E731
                                  stream_nbytes=t[2].reshape(2, 2))
    own, foreign = make((blob, st, nb)), make(R.to_foreign(blob, st, nb))
    assert own.has_frame_index is True and foreign.has_frame_index is False
    own._splice_layout(5, "append")  # (the layout test append and overwrite apply: unchanged)
    with pytest.raises(ValueError, match="libFLAC-written streams are not supported"):
        foreign._splice_layout(5, "append")
    with pytest.raises(ValueError, match="level 1 has block size 1152, the store's streams have 4096"):
        own._splice_layout(1, "append")
    part = fa.FlacArray(None, shape=data.shape, global_shape=(4, 2, n), compressed=blob, dtype=np.int32, stream_starts=st.reshape(2, 2),
                        stream_nbytes=nb.reshape(2, 2))
    with pytest.raises(NotImplementedError, match="one part of a distributed array"):
        part.reindex()
    for name in ("append", "overwrite", "frame_status", "salvage"):
        assert "reindex(" in getattr(fa.FlacArray, name).__doc__, name
