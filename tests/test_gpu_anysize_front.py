"""The frame pipeline of ResNet18-IBN-SE at any crop size on the MI355X (pytest -m gpu): any_front_kernel (csrc/anysize_front.hip),
reid_frame_submit_hw, reid_embed_frame_u8_hw and the stream classes with arch="seres18_hw".

  kernel    reid_debug_any_front, fused 1 against fused 0 (resize, generic GEMM stem, max-pool in three launches) BIT FOR BIT on every
            element, both within the float64 bound of tests/anysize_front_ref.py, guard row NaN, no NaN written, fault bits 0, an image's
            result independent of the batch.  Sizes: the table in anysize_front_ref.SIZES, sources (1, 1), (9, 300), (300, 200).
  entries   frame_submit_hw + frame_fetch and embed_frame_u8(size=) against embed_ragged_u8(size=), bit for bit.
  streams   CameraStream / MultiCameraStream / LookaheadCameraStream against the three blocking calls per frame, bit for bit.
  refusals  before the slot is touched: a frame submitted earlier still fetches with its own bits.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_front_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def sd0():
    return synth.seres18_state_dict(0)


@pytest.fixture(scope="module")
def blob0(sd0):
    return weights.pack_seres18(sd0)[:2]


@pytest.fixture(scope="module")
def stem(sd0):
    return ref.stem_of(sd0)


@pytest.fixture(scope="module")
def eng(blob0):
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.load_seres18(*blob0)
    yield e
    e.clear_fault()
    e.debug_switch("any_front", 2)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.set_chunk(1024)
    e.load_seres18(*blob0)


@pytest.fixture(scope="module")
def crops():
    return ref.crops()


@pytest.fixture(scope="module")
def pool_of_crops():
    return synth.ragged_crops_u8(9, seed=6)


# ----------------------------------------------------------------------------- 1. the kernel
def _front(eng, stem, crops, size, fused, **kw):
    out, guard = eng.debug_any_front(crops, size, stem[1], stem[2], stem[3], fused=fused, **kw)
    what = "%s fused=%d" % (size, fused)
    assert np.isnan(guard).all(), what + ": the guard row was written"
    assert not np.isnan(out).any(), what + ": an output was left unwritten (or is NaN)"
    assert eng.fault_bits() == 0
    return out


def _held(got, crop, size, stem, what, mean_std=None):
    want, b = ref.front64(crop, size[0], size[1], stem[0], stem[2], stem[3], mean_std)
    err = np.abs(got.astype(np.float64) - want)
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), float((err / b).max())))
    assert (err <= b).all(), "%s: err / bound %.3g" % (what, float((err / b).max()))


@pytest.mark.parametrize("size", ref.SIZES, ids=["%dx%d" % s for s in ref.SIZES])
def test_fused_front_equals_the_three_launches(eng, stem, crops, size):
    use = crops[2:] if size == (512, 512) else crops
    one = _front(eng, stem, use, size, 1)
    three = _front(eng, stem, use, size, 0)
    h2, w2 = ref.maps(*size)[2:]
    assert one.shape == three.shape == (len(use), h2, w2, 64)
    assert np.array_equal(_bits(one), _bits(three)), "%d of %d elements differ" % ((_bits(one) != _bits(three)).sum(), one.size)
    for i, crop in enumerate(use):
        _held(one[i], crop, size, stem, "%s source %s" % (size, crop.shape[:2]))
        if len(use) > 1:      # n = 1 against its place in n = 3
            assert np.array_equal(_bits(_front(eng, stem, [crop], size, 1)[0]), _bits(one[i])), i


def test_fused_front_with_another_mean_std(eng, stem, crops):
    size = (96, 72)
    one = _front(eng, stem, crops, size, 1, mean_std=ref.OTHER_MEAN_STD)
    assert np.array_equal(_bits(one), _bits(_front(eng, stem, crops, size, 0, mean_std=ref.OTHER_MEAN_STD)))
    assert not np.array_equal(_bits(one), _bits(_front(eng, stem, crops, size, 1)))
    for i, crop in enumerate(crops):
        _held(one[i], crop, size, stem, "mean_std source %s" % (crop.shape[:2],), ref.OTHER_MEAN_STD)


FRAME_H, FRAME_W = 120, 160
BOXES = np.array([[0, 0, 37, 51], [100, 60, 160, 120], [0, 80, 20, 120], [130, 0, 160, 9], [40, 30, 41, 31]], np.int32)   # all four borders


def test_fused_front_on_windows_of_a_frame(eng, stem):
    frame = np.random.default_rng(17).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    slices = [np.ascontiguousarray(frame[y1:y2, x1:x2]) for x1, y1, x2, y2 in BOXES]
    size = (57, 131)
    one = _front(eng, stem, BOXES, size, 1, frame=frame)
    assert np.array_equal(_bits(one), _bits(_front(eng, stem, BOXES, size, 0, frame=frame)))
    assert np.array_equal(_bits(one), _bits(_front(eng, stem, slices, size, 1)))
    for i, crop in enumerate(slices):
        _held(one[i], crop, size, stem, "window %s" % (BOXES[i],))


# ----------------------------------------------------------------------------- 2. the entries
def _frame_emb(eng, slot, crops, size, **kw):
    eng.frame_submit_hw(slot, crops, size, **kw)
    eng.frame_cost(slot, want_emb=True)
    emb, cost, iou = eng.frame_fetch(slot)
    assert cost is None and iou is None
    return emb


@pytest.mark.parametrize("hw_precision", [0, 2], ids=["f32", "f16x3"])
@pytest.mark.parametrize("size", [(128, 64), (96, 72)], ids=["128x64", "96x72"])
def test_frame_embeddings_equal_the_blocking_entry(eng, pool_of_crops, size, hw_precision):
    """m = 7 and m = 1 on both slots, m = 0, m = 5 in two passes (chunk 1: a pass holds 4 crops at either size), camera indices."""
    from reid_amd.engine import any_pass_size
    eng.set_hw_precision(hw_precision)
    crops = pool_of_crops
    want = eng.embed_ragged_u8(crops, size=size)
    for slot, m in ((0, 7), (1, 1)):
        got = _frame_emb(eng, slot, crops[:m], size)
        assert got.shape == (m, 512) and np.array_equal(_bits(got), _bits(want[:m])), (slot, m)
        assert eng.frame_dim(slot) == 512
    assert _frame_emb(eng, 0, [], size).shape == (0, 512)
    assert any_pass_size(1, *size) == 4
    eng.set_chunk(1)
    try:
        assert np.array_equal(_bits(_frame_emb(eng, 1, crops[:5], size)), _bits(want[:5]))
    finally:
        eng.set_chunk(1024)
    cams = np.asarray([2, 0, 5, 1], np.int32)
    eng.set_side_index(cams)
    with_cams = eng.embed_ragged_u8(crops[:4], size=size)
    eng.set_side_index(cams)
    got = _frame_emb(eng, 0, crops[:4], size)
    assert np.array_equal(_bits(got), _bits(with_cams)) and not np.array_equal(_bits(got), _bits(want[:4]))
    # another Normalize
    ms = ref.OTHER_MEAN_STD
    assert np.array_equal(_bits(_frame_emb(eng, 0, crops[:3], size, mean_std=ms)), _bits(eng.embed_ragged_u8(crops[:3], size=size, mean_std=ms)))
    assert eng.fault_bits() == 0


def test_windows_of_a_frame_equal_the_sliced_crops(eng):
    eng.set_hw_precision(2)
    frame = np.random.default_rng(18).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    slices = [np.ascontiguousarray(frame[y1:y2, x1:x2]) for x1, y1, x2, y2 in BOXES]
    for size in ((128, 64), (96, 72)):
        want_e, want_l = eng.embed_ragged_u8(slices, size=size, logits=True)
        got_e, got_l = eng.embed_frame_u8(frame, BOXES, logits=True, size=size)
        assert np.array_equal(_bits(got_e), _bits(want_e)) and np.array_equal(_bits(got_l), _bits(want_l)), size
    assert eng.embed_frame_u8(frame, BOXES[:0], size=(96, 72)).shape == (0, 512)


def test_debug_keep_and_the_switch_give_the_same_bits(eng, pool_of_crops):
    eng.set_hw_precision(2)
    size, crops = (96, 72), pool_of_crops[:3]
    want = eng.embed_ragged_u8(crops, size=size)
    h1, w1 = ref.maps(*size)[:2]
    eng.debug_keep(True)
    try:
        assert np.array_equal(_bits(_frame_emb(eng, 0, crops, size)), _bits(want))
        stage0 = eng.debug_stage(0, 3, size=size)
        assert stage0.size == 3 * h1 * w1 * 64 and np.isfinite(stage0).all()
    finally:
        eng.debug_keep(False)
    assert eng.debug_switch("any_front") == 2       # the default: the kernel for a pass this small (csrc/api.hip)
    try:
        for value in (0, 1):
            eng.debug_switch("any_front", value)
            assert np.array_equal(_bits(_frame_emb(eng, 1, crops, size)), _bits(want)), value
    finally:
        eng.debug_switch("any_front", 2)


def test_256x128_is_the_existing_entries(eng, pool_of_crops, blob0):
    crops = pool_of_crops[:4]
    frame = np.random.default_rng(19).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    eng.set_hw_precision(-1)
    try:
        for arch_blob in (blob0, weights.pack_seres18(synth.cares18_state_dict(0))[:2]):
            eng.set_precision(0)
            eng.load_seres18(*arch_blob)
            for mode in (0, 1, 2):
                eng.set_precision(mode)
                eng.frame_submit(0, crops)
                eng.frame_cost(0, want_emb=True)
                want = eng.frame_fetch(0)[0]
                assert np.array_equal(_bits(_frame_emb(eng, 1, crops, (256, 128))), _bits(want)), mode
                assert np.array_equal(_bits(eng.embed_frame_u8(frame, BOXES, size=(256, 128))), _bits(eng.embed_frame_u8(frame, BOXES))), mode
    finally:
        eng.set_precision(0)
        eng.load_seres18(*blob0)
    # another Normalize at 256 x 128: REID_ERR_ARG, as in reid_embed_ragged_u8_hw
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.frame_submit_hw(0, crops, (256, 128), mean_std=ref.OTHER_MEAN_STD)
    assert ei.value.status == -1


# ----------------------------------------------------------------------------- 3. the stream classes
SIZES_OF_FRAMES = [5, 7, 3, 6, 4, 6]
STREAM_SIZE, MAX_DIST, BUDGET = (128, 64), 0.2, 3


def _frames(crops, shift):
    return [[crops[(shift + 3 * f + i) % len(crops)] for i in range(m)] for f, m in enumerate(SIZES_OF_FRAMES)]


def _plan(f, m, tracks, base):
    """rows / targets of frame f's commit and the tracks alive after it: the matched prefix, and one new track per frame."""
    k = min(m, len(tracks))
    if k == m:
        return list(range(k)), tracks[:k], list(tracks)
    return list(range(k + 1)), tracks[:k] + [base + f], tracks + [base + f]


def _blocking(blob, frames, boxes, base):
    """The three blocking calls per frame on a context of its own: [(features, cost | None, iou | None)]."""
    from reid_amd.engine import Engine
    from reid_amd.iou_matching import iou_cost
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    e = Engine(0)
    log, tracks = [], []
    try:
        e.load_seres18(*blob)
        e.set_hw_precision("f16x3")
        met = NearestNeighborDistanceMetric("cosine", MAX_DIST, BUDGET, max_tracks=16, engine=e)
        for f, crops in enumerate(frames):
            m = len(crops)
            feats = e.embed_ragged_u8(crops, size=STREAM_SIZE)
            cost = met.distance(feats, tracks, max_distance=MAX_DIST) if tracks else None
            iou = iou_cost(boxes[:len(tracks)], boxes[:m]) if tracks else None
            rows, tg, after = _plan(f, m, tracks, base)
            met.partial_fit(feats[rows], tg, after)
            log.append((feats, cost, iou, list(tracks), rows, tg, after))
            tracks = after
        met.close()
    finally:
        e.close()
    return log


def _same(got, want, what):
    feats, cost, iou = got
    assert np.array_equal(_bits(feats), _bits(want[0])), what + ": features"
    if want[1] is not None:
        np.testing.assert_array_equal(cost, want[1], err_msg=what + ": appearance cost")
        np.testing.assert_array_equal(iou, want[2], err_msg=what + ": DIoU cost")


def test_streams_equal_the_three_blocking_calls(eng, pool_of_crops, blob0):
    from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream
    rng = np.random.default_rng(2)
    boxes = np.concatenate([rng.uniform(0, 200, (16, 2)), rng.uniform(10, 60, (16, 2))], 1)
    frames = {"A": _frames(pool_of_crops, 0), "B": _frames(pool_of_crops, 4)}
    want = {"A": _blocking(blob0, frames["A"], boxes, 50), "B": _blocking(blob0, frames["B"], boxes, 70)}
    assert sum(w[1].size for w in want["A"] if w[1] is not None) > 50
    kw = dict(max_dist=MAX_DIST, budget=BUDGET, max_tracks=16, arch="seres18_hw", size=STREAM_SIZE, hw_precision="f16x3")

    cam = CameraStream(*blob0, **kw)
    try:
        assert cam.eng.hw_precision == 2
        cam.submit(frames["A"][0])
        for f, (_, _, _, tracks, rows, tg, after) in enumerate(want["A"]):
            m = len(frames["A"][f])
            got = cam.step(tracks, boxes[:len(tracks)], boxes[:m], frames["A"][f + 1] if f + 1 < 6 else None)
            _same(got, want["A"][f], "CameraStream frame %d" % f)
            cam.commit(rows, tg, after)
    finally:
        cam.close(destroy=True)

    cams = MultiCameraStream(*blob0, 2, **kw)
    try:
        cams.submit([frames["A"][0], frames["B"][0]])
        for f in range(6):
            cur = [want["A"][f], want["B"][f]]
            ms = [len(frames["A"][f]), len(frames["B"][f])]
            res = cams.step([c[3] for c in cur], [boxes[:len(c[3])] for c in cur], [boxes[:m] for m in ms],
                            [frames["A"][f + 1], frames["B"][f + 1]] if f + 1 < 6 else None)
            for c in range(2):
                _same(res[c], cur[c], "MultiCameraStream camera %d frame %d" % (c, f))
            cams.commit([c[4] for c in cur], [c[5] for c in cur], [c[6] for c in cur])
    finally:
        cams.close(destroy=True)

    la = LookaheadCameraStream(*blob0, frames_per_pass=2, **kw)
    try:
        groups = [frames["A"][i:i + 2] for i in range(0, 6, 2)]
        la.submit_group(groups[0])
        for g in range(3):
            for j in range(2):
                f = 2 * g + j
                _, _, _, tracks, rows, tg, after = want["A"][f]
                nxt = groups[g + 1] if j == la.handover and g + 1 < 3 else None
                got = la.step(j, tracks, boxes[:len(tracks)], boxes[:len(frames["A"][f])], next_group=nxt)
                _same(got, want["A"][f], "LookaheadCameraStream frame %d" % f)
                la.commit(j, rows, tg, after)
    finally:
        la.close(destroy=True)


# ----------------------------------------------------------------------------- 4. refusals
def _raw_submit(e, crops, out_h, out_w):
    slab, offs, hw, n = e._frame_pack(1, crops)
    return e.lib.reid_frame_submit_hw(e.h, 1, _p(slab), _p(offs), _p(hw), n, out_h, out_w, None)


def test_refusals_come_before_the_slot_is_touched(eng, pool_of_crops, blob0):
    crops, size = pool_of_crops[:3], (128, 64)
    eng.set_precision(0)
    eng.set_hw_precision(2)
    want = eng.embed_ragged_u8(crops, size=size)

    def pending_frame_survives(refuse, status, *words):
        eng.set_precision(0)
        eng.set_hw_precision(2)
        eng.load_seres18(*blob0)
        eng.frame_submit_hw(1, crops, size)
        eng.frame_cost(1, want_emb=True)
        got = refuse()
        msg = eng.lib.reid_last_error().decode()
        assert got == status and all(w in msg for w in words), (got, msg)
        assert np.array_equal(_bits(eng.frame_fetch(1)[0]), _bits(want)), msg

    try:
        pending_frame_survives(lambda: _raw_submit(eng, crops, 31, 64), -1, "31")
        pending_frame_survives(lambda: _raw_submit(eng, crops, 128, 513), -1, "513")

        def sibling():
            eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
            return _raw_submit(eng, crops, 128, 64)
        pending_frame_survives(sibling, -1, "cares18_ibn")

        def mode2_without_the_setting():
            eng.set_hw_precision(-1)
            eng.set_precision(2)
            return _raw_submit(eng, crops, 128, 64)
        pending_frame_survives(mode2_without_the_setting, -1, "mode 2")
    finally:
        eng.set_precision(0)
        eng.set_hw_precision(-1)
        eng.load_seres18(*blob0)
    assert eng.fault_bits() == 0


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
crops = synth.ragged_crops_u8(3, seed=6)
before = eng.embed_ragged_u8(crops, size=(128, 64))
eng.frame_submit(1, crops)
eng.frame_cost(1, want_emb=True)
try:
    eng.frame_submit_hw(1, crops, (128, 64))
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_anysize_front.so" in str(e)
    ok = ok and np.array_equal(eng.frame_fetch(1)[0], eng.embed_ragged_u8(crops))
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.embed_ragged_u8(crops, size=(128, 64)), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_submit(tmp_path):
    """A copy of the build without libreid_hip_anysize_front.so, loaded through REID_HIP_LIB in a fresh child process: the submit is
    REID_ERR_STATE naming the file, the frame submitted before it fetches with its own bits, and the blocking entry works before and after."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_anysize_front.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED -3" in r.stdout and lib in r.stdout
