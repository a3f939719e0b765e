"""The host entry points of the ResNet18-SE family (csrc/api.hip) on the MI355X (pytest -m gpu): what the shared host skeleton
(RaggedSrc, EmbedOut, embed_host: csrc/reid_internal.h) must keep bit for bit - windows of a frame in several passes, ragged crops
whose metadata arrays do not lie one behind the other, a packing that is not crop after crop - and the statuses decided on the host.
Every comparison is array_equal: the paths compared run the same kernels on the same pixels."""
import ctypes as C

import numpy as np
import pytest

from reid_amd import synth, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    yield e
    e.debug_switch("host_pipeline", 1)
    e.set_chunk(1024)
    e.set_precision(0)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("precision", [0, 2])
def test_frame_entry_in_several_passes_with_logits(eng, precision):
    """reid_embed_frame_u8 with more boxes than a pass holds (5 boxes, passes of 2; one box touches the frame's border, one is 3 pixels
    wide), unpipelined and pipelined: embeddings and logits equal the one-pass call's and those of reid_embed_ragged_u8 on the same
    pixels sliced on the host."""
    frame = np.random.default_rng(23).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    boxes = np.asarray([[70, 125, 130, 275], [0, 0, 40, 60], [590, 400, 640, 480], [319, 90, 322, 390], [256, 112, 384, 368]], np.int32)
    crops = [frame[y1:y2, x1:x2] for x1, y1, x2, y2 in boxes]
    assert crops[3].shape[1] == 3
    eng.set_precision(precision)
    try:
        eng.set_chunk(1024)
        want_e, want_l = eng.embed_frame_u8(frame, boxes, logits=True)
        assert np.isfinite(want_e).all() and np.isfinite(want_l).all() and want_l.shape[0] == 5
        rag_e, rag_l = eng.embed_ragged_u8(crops, logits=True)
        assert np.array_equal(rag_e, want_e) and np.array_equal(rag_l, want_l)
        eng.set_chunk(2)
        sliced_e, sliced_l = eng.embed_ragged_u8(crops, logits=True)
        for pipeline in (0, 1):
            eng.debug_switch("host_pipeline", pipeline)
            e, lg = eng.embed_frame_u8(frame, boxes, logits=True)
            print("FRAME passes of 2, host_pipeline %d, precision %d: max |emb - one pass| %.3g, max |logits - one pass| %.3g" %
                  (pipeline, precision, np.abs(e - want_e).max(), np.abs(lg - want_l).max()))
            assert np.array_equal(e, sliced_e) and np.array_equal(lg, sliced_l), "host_pipeline %d: frame against sliced crops" % pipeline
            assert np.array_equal(e, want_e) and np.array_equal(lg, want_l), "host_pipeline %d: passes of 2 against one pass" % pipeline
            assert np.array_equal(eng.embed_frame_u8(frame, boxes), want_e)      # without logits
    finally:
        eng.debug_switch("host_pipeline", 1)
        eng.set_chunk(1024)
        eng.set_precision(0)


def _raw_ragged(eng, packed, offsets, hw, n, logits=True):
    """reid_embed_ragged_u8 on the arrays as they are (ctypes arrays or numpy); returns (status, emb, logits)."""
    emb = np.full((n, 512), 7.0, np.float32)
    lg = np.full((n, eng.num_class), 7.0, np.float32) if logits else None
    addr = lambda a: a if a is None or isinstance(a, C.c_void_p) else (_p(a) if isinstance(a, np.ndarray) else C.cast(a, C.c_void_p))
    return eng.lib.reid_embed_ragged_u8(eng.h, addr(packed), addr(offsets), addr(hw), n, _p(emb), _p(lg)), emb, lg


def _pack(crops, order):
    """The crops laid into one buffer in `order`; offsets / hw stay in the crops' own order."""
    offsets = np.empty(len(crops), np.int64)
    at = 0
    for i in order:
        offsets[i] = at
        at += crops[i].size
    packed = np.empty(at, np.uint8)
    for i, c in enumerate(crops):
        packed[offsets[i]: offsets[i] + c.size] = c.reshape(-1)
    return packed, offsets, np.asarray([c.shape[:2] for c in crops], np.int32)


@pytest.mark.parametrize("chunk", [1024, 3], ids=["one_pass", "passes_of_3"])
def test_ragged_entry_separate_metadata_arrays_and_reversed_packing(eng, chunk):
    """reid_embed_ragged_u8 with hw directly behind offsets (one metadata copy) against two separately allocated ctypes arrays (two
    copies), and against a buffer packed from the last crop to the first - a later pass's byte span then lies below an earlier one's."""
    n = 7
    crops = synth.ragged_crops_u8(n, 31)
    packed, offsets, hw = _pack(crops, range(n))
    block = (C.c_int64 * (2 * n))()                       # [offsets n x 8 | hw n x 8]
    C.memmove(block, offsets.ctypes.data, n * 8)
    C.memmove(C.addressof(block) + n * 8, hw.ctypes.data, n * 8)
    far_off = (C.c_int64 * n)(*offsets.tolist())
    gap = (C.c_int64 * 64)()                              # keeps the two arrays apart
    far_hw = (C.c_int32 * (2 * n))(*hw.reshape(-1).tolist())
    assert C.addressof(far_hw) != C.addressof(far_off) + n * 8 and len(gap) == 64
    eng.set_precision(0)
    eng.set_chunk(chunk)
    try:
        st, want_e, want_l = _raw_ragged(eng, packed, block, C.c_void_p(C.addressof(block) + n * 8), n)
        assert st == 0 and np.isfinite(want_e).all() and np.isfinite(want_l).all()
        st, e, lg = _raw_ragged(eng, packed, far_off, far_hw, n)
        assert st == 0 and np.array_equal(e, want_e) and np.array_equal(lg, want_l)
        rpacked, roffsets, rhw = _pack(crops, range(n - 1, -1, -1))
        assert roffsets[0] > roffsets[-1] == 0
        st, e, lg = _raw_ragged(eng, rpacked, roffsets, rhw, n)
        assert st == 0 and np.array_equal(e, want_e) and np.array_equal(lg, want_l)
        assert np.array_equal(eng.embed_ragged_u8(crops), want_e)
    finally:
        eng.set_chunk(1024)


def test_refusals_of_the_seres18_entries_come_from_the_host(eng):
    """n == 0 is REID_OK and writes nothing, with or without weights; a crop without pixels or with a negative offset, an empty or
    out-of-frame box are REID_ERR_ARG (-1); no weights is REID_ERR_STATE (-3).  The fault word stays clear and the next call works."""
    from reid_amd.engine import Engine
    crops = synth.ragged_crops_u8(3, 5)
    packed, offsets, hw = _pack(crops, range(3))
    dense = synth.crops_u8(2, 3)
    frame = np.zeros((60, 80, 3), np.uint8)
    box = np.asarray([[1, 2, 30, 50]], np.int32)
    eng.set_precision(0)
    want = eng.embed_ragged_u8(crops)

    def empties(e):
        emb, lg = np.full((2, 512), 7.0, np.float32), np.full((2, max(e.num_class, 1)), 7.0, np.float32)
        x = np.zeros((1, 3, 256, 128), np.float32)
        assert e.lib.reid_embed_u8(e.h, _p(dense), 0, _p(emb), _p(lg)) == 0
        assert e.lib.reid_embed_f32_nchw(e.h, _p(x), 0, _p(emb), _p(lg)) == 0
        assert e.lib.reid_embed_ragged_u8(e.h, _p(packed), _p(offsets), _p(hw), 0, _p(emb), _p(lg)) == 0
        assert e.lib.reid_embed_frame_u8(e.h, _p(frame), 60, 80, _p(box), 0, _p(emb), _p(lg)) == 0
        assert (emb == 7.0).all() and (lg == 7.0).all()

    empties(eng)
    for bad_hw, bad_off in (([[0, 5]], None), ([[5, 0]], None), (None, -3)):
        h2, o2 = hw.copy(), offsets.copy()
        if bad_hw:
            h2[1] = bad_hw[0]
        else:
            o2[2] = bad_off
        assert _raw_ragged(eng, packed, o2, h2, 3)[0] == -1
    for bad_box in ([10, 10, 10, 50], [10, 10, 40, 10], [0, 0, 81, 50], [0, 0, 40, 61], [-1, 0, 40, 50]):
        b = np.asarray([box[0], bad_box], np.int32)
        emb = np.empty((2, 512), np.float32)
        assert eng.lib.reid_embed_frame_u8(eng.h, _p(frame), 60, 80, _p(b), 2, _p(emb), None) == -1
    fresh = Engine(0)                                            # a second context, without weights
    try:
        empties(fresh)
        emb = np.empty((2, 512), np.float32)
        assert fresh.lib.reid_embed_u8(fresh.h, _p(dense), 2, _p(emb), None) == -3
        assert b"reid_seres18_load" in fresh.lib.reid_last_error()
        assert fresh.fault_bits() == 0
    finally:
        fresh.close()
    assert eng.fault_bits() == 0
    eng.device_sync()
    np.testing.assert_array_equal(eng.embed_ragged_u8(crops), want)
