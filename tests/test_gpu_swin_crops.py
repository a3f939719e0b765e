"""Swin-T from uint8 crops and frame windows on the MI355X (pytest -m gpu): the fused front kernel alone against float64
(tests/swin_crops_ref.py holds the restatement and the derivation of its bound), the fused path against the two-step path bit for bit,
passes, the Extractor with a Swin checkpoint in a tracker's metric, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import nn_matching as onm
from reid_amd import _ffi, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_crops_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

NUM_CLASS = 8
VIEWS = 3


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.set_precision(0)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def cs():
    return ref.crop_set()


@pytest.fixture(scope="module")
def sds():
    return {"v1": synth.swin_state_dict(0, num_class=NUM_CLASS), "v2": synth.swin_state_dict(0, num_class=NUM_CLASS, version="v2"),
            "views": synth.swin_state_dict(0, num_class=NUM_CLASS, views=VIEWS)}


@pytest.fixture(scope="module")
def blobs(sds):
    return {k: weights.pack_swin(sd)[:2] for k, sd in sds.items()}


def _load(eng, blobs, key, mode):
    eng.set_precision(0)
    eng.load_swin(*blobs[key])
    eng.set_precision(mode)


def _two_step(eng, crops, size=(224, 224), side=None):
    """(emb, logits, sfe tap) of reid_swin_embed_f32_nchw on the host-preprocessed crops."""
    if side is not None:
        eng.set_side_index(side)
    emb, lg = eng.swin_embed_f32_nchw(ref.preprocess(crops, size), logits=True)
    return emb, lg, eng.debug_swin_stage(0, len(crops), *size)


# ----------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("size,mean_std", [((224, 224), None), ((448, 224), None), ((224, 224), ref.OTHER_MEAN_STD)],
                         ids=["224x224", "448x224", "224x224-other-mean-std"])
def test_front_kernel_alone(eng, cs, size, mean_std):
    """swin_crop_front_kernel on the packed crops and on the same crops as windows of the frame (pitch 640): the same bits, each within the
    derived bound of float64 (module docstring of swin_crops_ref), and the bits of sfe_conv1_kernel on the host-preprocessed image."""
    frame, crops, boxes = cs
    mean, std = (ref.IMAGENET_MEAN, ref.IMAGENET_STD) if mean_std is None else (mean_std[:3], mean_std[3:])
    w, b = ref.conv_weights()
    eng.set_precision(0)
    pk, offsets, hw = ref.packed(crops)
    got = eng.debug_swin_crop_front(pk, offsets, hw, w, b, size=size, mean_std=mean_std)
    assert got.shape == (len(crops), size[0] // 2, size[1] // 2, 12) and np.isfinite(got).all()    # NaN fill: every element written
    f_off = np.array([(y * ref.FRAME_W + x) * 3 for y, x in ref.CROP_YX], np.int64)
    from_frame = eng.debug_swin_crop_front(frame, f_off, hw, w, b, size=size, mean_std=mean_std, pitch=ref.FRAME_W)
    np.testing.assert_array_equal(from_frame, got, err_msg="windows of a frame against packed crops")
    worst = 0.0
    for i, crop in enumerate(crops):
        want, bound = ref.front64(crop, w, b, size, mean, std)
        err = np.abs(got[i].astype(np.float64) - want)
        at = np.unravel_index(np.argmax(err / bound), err.shape)
        worst = max(worst, float((err / bound)[at]))
        print("RATIO swin_crop_front %s crop %dx%d worst err/bound %.4f" % (size, crop.shape[0], crop.shape[1], (err / bound)[at]))
        assert (err <= bound).all(), "crop %s at %s: got %r, float64 %r, bound %g" % (crop.shape, at, got[i][at], want[at], bound[at])
    assert worst > 0.0
    two_step = eng.debug_swin_conv1(ref.preprocess(crops, size, mean, std), w, b)
    np.testing.assert_array_equal(got, two_step, err_msg="fused front end against preprocess + sfe_conv1_kernel")


# ----------------------------------------------------------------------------- 2. fused path == two-step path
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_fused_path_equals_two_step_path(eng, cs, blobs, version, mode):
    """Embeddings, logits and the SFE tap of the ragged and the frame entry are the two-step path's, bit for bit, in every mode."""
    frame, crops, boxes = cs
    _load(eng, blobs, version, mode)
    try:
        emb, lg, sfe = _two_step(eng, crops)
        assert np.isfinite(emb).all() and emb.shape == (len(crops), 96) and lg.shape == (len(crops), NUM_CLASS)
        e1, l1 = eng.swin_embed_ragged_u8(crops, logits=True)
        s1 = eng.debug_swin_stage(0, len(crops))
        e2, l2 = eng.swin_embed_frame_u8(frame, boxes, logits=True)
        s2 = eng.debug_swin_stage(0, len(crops))
        e3 = eng.swin_embed_ragged_u8(crops)                                       # without logits
    finally:
        eng.set_precision(0)
    for what, (e, l, s) in (("ragged", (e1, l1, s1)), ("frame", (e2, l2, s2))):
        np.testing.assert_array_equal(s, sfe, err_msg="%s: swin.sfe tap" % what)
        np.testing.assert_array_equal(e, emb, err_msg="%s: embeddings" % what)
        np.testing.assert_array_equal(l, lg, err_msg="%s: logits" % what)
    np.testing.assert_array_equal(e3, emb)


def test_fused_path_at_448x224(eng, cs, blobs):
    frame, crops, boxes = cs
    size = (448, 224)
    _load(eng, blobs, "v1", 2)
    try:
        emb, lg, sfe = _two_step(eng, crops[3:8], size)
        e1, l1 = eng.swin_embed_ragged_u8(crops[3:8], size=size, logits=True)
        s1 = eng.debug_swin_stage(0, 5, *size)
        e2, l2 = eng.swin_embed_frame_u8(frame, boxes[3:8], size=size, logits=True)
        at_224 = eng.swin_embed_ragged_u8(crops[3:8])
    finally:
        eng.set_precision(0)
    np.testing.assert_array_equal(s1, sfe)
    for e, l in ((e1, l1), (e2, l2)):
        np.testing.assert_array_equal(e, emb)
        np.testing.assert_array_equal(l, lg)
    assert not np.array_equal(emb, at_224)                                        # the size did reach the kernel


def test_fused_path_with_a_view_index(eng, cs, blobs):
    """reid_ctx_set_side_index belongs to the common body: it applies to the crops entries as to the float one, over several passes too."""
    frame, crops, boxes = cs
    side = np.arange(len(crops)) % VIEWS
    _load(eng, blobs, "views", 2)
    try:
        emb, lg, sfe = _two_step(eng, crops, side=side)
        plain = eng.swin_embed_ragged_u8(crops)
        eng.set_side_index(side)
        e1 = eng.swin_embed_ragged_u8(crops)
        s1 = eng.debug_swin_stage(0, len(crops))
        eng.set_side_index(side)
        e2 = eng.swin_embed_frame_u8(frame, boxes)
        eng.set_chunk(4)
        eng.set_side_index(side)
        e3 = eng.swin_embed_ragged_u8(crops)
    finally:
        eng.set_side_index(None)
        eng.set_chunk(1024)
        eng.set_precision(0)
    np.testing.assert_array_equal(s1, sfe)
    for e in (e1, e2, e3):
        np.testing.assert_array_equal(e, emb)
    assert not np.array_equal(plain, emb)


# ----------------------------------------------------------------------------- 3. passes
@pytest.mark.parametrize("pipeline", [1, 0], ids=["pipelined", "unpipelined"])
def test_passes_leave_the_bits_alone(eng, cs, blobs, pipeline):
    """5 crops in passes of 2 (reid_ctx_set_chunk, and the Swin pass cap) equal the one-pass result, with the host pipeline on and off."""
    frame, crops, boxes = cs
    sel = [8, 1, 5, 6, 4]
    five, five_boxes = [crops[i] for i in sel], boxes[sel]
    _load(eng, blobs, "v1", 2)
    try:
        one, one_lg = eng.swin_embed_ragged_u8(five, logits=True)
        eng.debug_switch("host_pipeline", pipeline)
        eng.set_chunk(2)
        got, got_lg = eng.swin_embed_ragged_u8(five, logits=True)
        got_frame = eng.swin_embed_frame_u8(frame, five_boxes)
        eng.set_chunk(1024)
        eng.debug_switch("swin_chunk_cap", 2)
        capped = eng.swin_embed_ragged_u8(five)
    finally:
        eng.debug_switch("swin_chunk_cap", 1024)
        eng.debug_switch("host_pipeline", 1)
        eng.set_chunk(1024)
        eng.set_precision(0)
    np.testing.assert_array_equal(got, one)
    np.testing.assert_array_equal(got_lg, one_lg)
    np.testing.assert_array_equal(got_frame, one)
    np.testing.assert_array_equal(capped, one)


# ----------------------------------------------------------------------------- 4. Extractor
def test_extractor_with_a_swin_checkpoint(eng, cs, sds, blobs):
    """Extractor(swin state_dict): [N, 96] from a list of crops, from a stacked uint8 array and from_frame (clipped like the ResNet
    one), equal to the engine's arrays in the extractor's arithmetic; the features drive NearestNeighborDistanceMetric like the oracle's
    metric, to test_gpu_bank.py's bound for the bank cost; a ResNet Extractor made afterwards is untouched by it."""
    from reid_amd.extractor import Extractor
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    frame, crops, boxes = cs
    ext = Extractor(sds["v1"], precision="f16x3")
    assert ext.size == (224, 224) and ext.precision == "f16x3"
    feats = ext(crops)
    stacked = np.stack([crops[4], crops[4][::-1].copy()])
    f_stacked = ext(stacked)
    xywh = np.array([[320.0, 240.0, 100.0, 200.0], [10.0, 20.0, 60.0, 90.0], [630.0, 470.0, 50.0, 40.0]])      # two of them clipped
    xyxy = np.array([(max(int(x - w / 2), 0), max(int(y - h / 2), 0), min(int(x + w / 2), ref.FRAME_W - 1), min(int(y + h / 2), ref.FRAME_H - 1))
                     for x, y, w, h in xywh], np.int32)
    assert xyxy[1, 0] == 0 and xyxy[1, 1] == 0 and xyxy[2, 2] == ref.FRAME_W - 1 and xyxy[2, 3] == ref.FRAME_H - 1
    f_frame = ext.from_frame(xywh, frame)
    assert ext.from_frame(np.zeros((0, 4)), frame).size == 0
    assert eng.precision == 0                                    # the shared engine got its mode back
    _load(eng, blobs, "v1", 2)
    try:
        want = eng.swin_embed_f32_nchw(ref.preprocess(crops))
        want_stacked = eng.swin_embed_f32_nchw(ref.preprocess(list(stacked)))
        want_frame = eng.swin_embed_f32_nchw(ref.preprocess([frame[y1:y2, x1:x2] for x1, y1, x2, y2 in xyxy]))
    finally:
        eng.set_precision(0)
    eng._swin_owner = None                                       # this test loaded other (equal) weights over the extractor's
    for got, w in ((feats, want), (f_stacked, want_stacked), (f_frame, want_frame)):
        assert got.dtype == np.float32 and got.shape == w.shape and got.shape[1] == 96 and got.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(got, w)
    # a tracker's metric on these features: tracks 0 .. 2 get three samples each, the other three crops are the detections
    metric = NearestNeighborDistanceMetric("cosine", 0.2, budget=5, engine=eng)
    orc = onm.NearestNeighborDistanceMetric("cosine", 0.2, 5)
    try:
        targets = [0, 1, 2, 0, 1, 2]
        metric.partial_fit(feats[:6], targets, [0, 1, 2])
        orc.partial_fit(feats[:6].astype(np.float64), targets, [0, 1, 2])
        got = np.asarray(metric.distance(feats[6:], [2, 0, 1]), np.float64)
        ref_cost = np.asarray(orc.distance(feats[6:].astype(np.float64), [2, 0, 1]), np.float64)
    finally:
        metric.close()
    n = -(-96 // 64) + 8                                         # test_gpu_bank.py: (2n + 6) u, n = ceil(d / 64) + 8 roundings, SAFETY 2
    assert got.shape == ref_cost.shape == (3, 3)
    assert (np.abs(got - ref_cost) <= 2.0 * (2 * n + 6) * 2.0 ** -24).all(), np.abs(got - ref_cost).max()
    # a ResNet extractor created afterwards, used before and after another Swin call
    rsd = synth.seres18_state_dict(0)
    rext = Extractor(rsd, precision="f16x3")
    assert rext.size == (128, 256)
    r1 = rext(crops)
    again = ext(crops)
    r2 = rext(crops)
    assert eng.precision_ok(0, 2) and eng.precision_ok(1, 2)
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(rsd)[:2])
    eng.set_precision(2)
    try:
        r_want = eng.embed_ragged_u8(crops)
    finally:
        eng.set_precision(0)
    assert r1.shape == (len(crops), 512) and r1.dtype == np.float32
    np.testing.assert_array_equal(r1, r_want)
    np.testing.assert_array_equal(r2, r_want)
    np.testing.assert_array_equal(again, want)
    with pytest.raises(ValueError):
        Extractor(rsd, size=(224, 224))


# ----------------------------------------------------------------------------- 5. refusals
def _raw_ragged(eng, h, crops, out_h=224, out_w=224, mean_std=None):
    pk, offsets, hw = ref.packed(crops)
    emb = np.empty((len(crops), 96), np.float32)
    ms = None if mean_std is None else np.ascontiguousarray(mean_std, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return eng.lib.reid_swin_embed_ragged_u8(h, p(pk), p(offsets), p(hw), len(crops), out_h, out_w, p(ms), p(emb), None)


def _raw_frame(eng, h, frame, boxes, out_h=224, out_w=224):
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    emb = np.empty((len(boxes), 96), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return eng.lib.reid_swin_embed_frame_u8(h, p(frame), frame.shape[0], frame.shape[1], p(boxes), len(boxes), out_h, out_w, None, p(emb), None)


def test_refusals_come_from_the_host(eng, cs, blobs):
    """Bad arguments are REID_ERR_ARG (-1) and a context without Swin weights REID_ERR_STATE (-3), decided on the host before any
    launch: the fault word stays clear and the next call works."""
    from reid_amd.engine import Engine
    frame, crops, boxes = cs
    _load(eng, blobs, "v1", 0)
    want = eng.swin_embed_ragged_u8(crops[:2])
    assert _raw_ragged(eng, eng.h, crops[:2], out_h=200) == -1
    assert _raw_ragged(eng, eng.h, crops[:2], out_w=100) == -1
    assert _raw_frame(eng, eng.h, frame, boxes[:2], out_h=200) == -1
    assert _raw_ragged(eng, eng.h, crops[:2], mean_std=[0.5, 0.5, 0.5, 0.2, 0.0, 0.2]) == -1          # std = 0
    assert _raw_ragged(eng, eng.h, crops[:2], mean_std=[0.5, 0.5, 0.5, 0.2, -0.1, 0.2]) == -1
    assert _raw_frame(eng, eng.h, frame, [[600, 400, 641, 470]]) == -1                                # beyond the frame
    assert _raw_frame(eng, eng.h, frame, [[10, 10, 20, 481]]) == -1
    assert _raw_frame(eng, eng.h, frame, [[-1, 10, 20, 40]]) == -1
    assert _raw_frame(eng, eng.h, frame, [[30, 10, 30, 40]]) == -1                                    # empty
    assert _raw_frame(eng, eng.h, frame, [[30, 40, 60, 40]]) == -1
    with pytest.raises(ValueError):
        eng.swin_embed_ragged_u8(crops[:2], size=(200, 224))
    with pytest.raises(ValueError):
        eng.swin_embed_ragged_u8(crops[:2], mean_std=[0.5, 0.5, 0.5, 0.2, 0.0, 0.2])
    fresh = Engine(0)                                            # a second context, without Swin weights
    try:
        assert _raw_ragged(fresh, fresh.h, crops[:2]) == -3
        assert _raw_frame(fresh, fresh.h, frame, boxes[:2]) == -3
        assert b"reid_swin_load" in fresh.lib.reid_last_error()
        assert fresh.fault_bits() == 0
    finally:
        fresh.close()
    assert eng.fault_bits() == 0
    eng.device_sync()
    np.testing.assert_array_equal(eng.swin_embed_ragged_u8(crops[:2]), want)
    assert eng.swin_embed_frame_u8(frame, np.zeros((0, 4), np.int32)).shape == (0, 96)


# ----------------------------------------------------------------------------- 6. without the library
_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0, num_class=8))[:2])
x = synth.images_f32(1, 1)
before = eng.swin_embed_f32_nchw(x)
try:
    eng.swin_embed_ragged_u8([np.zeros((5, 4, 3), np.uint8)])
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_swin_crops.so" in str(e)
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.swin_embed_f32_nchw(x), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_crops_call(tmp_path):
    """A copy of the package without libreid_hip_swin_crops.so, in a fresh child process: a crops call returns REID_ERR_STATE naming the
    library before anything is launched, and the float entry works before and after it."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_swin_crops.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                       env=dict(os.environ))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED -3" in r.stdout and lib in r.stdout
