"""ResNet18-IBN-SE at any input size in fp16 storage with fp32 accumulation on the MI355X (pytest -m gpu tests/test_gpu_anysize_f16.py).

Kernels of libreid_hip_anysize_f16.so through the launchers the forward calls (reid_debug_any_*_f16), against the float64 oracles and
the bounds of tests/anysize_f16_ref.py (its module docstring derives them):
  * any_conv_f16_kernel on the eleven geometries of tests/anysize_x3_ref.py: random f16 operands with the epilogue on within
    e32 + H (|v| + e32) + 2^-25; small integers bit for bit; the tile form follows the geometry; an image's rows have the same bits at
    any position and any n;
  * stem + max-pool at (33, 47) and (64, 32): the stem within the same kind of bound (K = 147), the pool bit for bit the numpy maximum of
    the stored f16 map;
  * the three tails at hw in (4, 8, 30, 108, 238), c in (64, 512), n = 3: fp32 statistics error + one f16 rounding; what a launch must
    leave alone comes back as NaN; out aliasing y gives the same bits.
Every output has a guard row that must still read as NaN, and the fault word stays 0.

Forward: reid_ctx_set_hw_f16(1) on the three cases of tests/golden/anysize.npz under the mode-1 limits of tests/test_gpu_parity.py
(1 - cos < 1e-4; embeddings, logits and stage taps within 2e-2 of the largest magnitude), other bits than hw_precision 0 and 2; the
equalities (pass sizes, host / device entries, uint8 / PIL floats, frame windows / ragged crops, CameraStream / blocking calls) bit for
bit; the setting's rules; a build without the side library.

Measured on the MI355X (as fractions of the quantities the limits above are set on; the limits are not tightened to them):
  (64, 32):    1 - cos 1.8e-07, emb 1.1e-03, logits 5.1e-04, worst stage 1.4e-03, TTA descriptor 1 - cos 1.2e-07
  (96, 72):    1 - cos 1.8e-07, emb 4.9e-04, logits 4.6e-04, worst stage 1.4e-03, TTA descriptor 1 - cos 1.2e-07
  (224, 268):  1 - cos 2.4e-07, emb 5.4e-04, logits 3.4e-04, worst stage 1.5e-03, TTA descriptor 1 - cos below fp32's resolution
  kernels, worst err / bound: convolution 0.96, stem 0.92, IBN finish 0.995, SE tail 0.99, SE gate 0.06, GeM 0.15, neck 0.40.  The
  f16-stored outputs come close to 1 by construction: H |v| is the half-ulp of a value at the bottom of its binade, and among thousands of
  outputs some lie there and round by almost half an ulp; the fp32 part of those bounds is two orders of magnitude smaller."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import seres18
from reid_amd import _ffi, synth, weights
from reid_amd.engine import stage_shapes
from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_f16_ref as r  # noqa: E402
import anysize_ref  # noqa: E402
import pil_resize_ref  # noqa: E402
import test_gpu_anysize as base  # noqa: E402

pytestmark = [pytest.mark.gpu]

_bits, _p = base._bits, base._p
SIZE = (96, 72)


def _bits16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


@pytest.fixture(scope="module")
def sd0():
    return synth.seres18_state_dict(0)


@pytest.fixture(scope="module")
def blob0(sd0):
    return weights.pack_seres18(sd0)[:2]


def _defaults(e):
    e.clear_fault()
    e.debug_switch("anysize_force", 0)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.set_hw_siblings(False)
    e.set_hw_ema(False)
    e.set_hw_f16(False)               # without the feature the module fails here, at its first use of reid_ctx_set_hw_f16
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def eng(blob0):
    from reid_amd.engine import get_engine
    e = get_engine(0)
    _defaults(e)
    e.load_seres18(*blob0)
    yield e
    _defaults(e)
    e.load_seres18(*blob0)


@pytest.fixture()
def eng_w0(eng, blob0):
    _defaults(eng)
    eng.load_seres18(*blob0)
    yield eng
    assert eng.fault_bits() == 0
    _defaults(eng)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anysize.npz"))


def _held(got, want, b, what):
    assert not np.isnan(got).any(), what + ": an output was left unwritten (or is NaN)"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / b).max())
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), worst))
    assert (err <= b).all(), "%s: err / bound %.3g" % (what, worst)


# ---------------------------------------------------------------------------------------------- 1. the convolution kernel
def _conv(eng, name, x, wt, stride, **kw):
    cout = r.GEOMS[name][1]
    out, guard, form = eng.debug_any_conv_f16(x, wt, stride, **kw)
    assert np.isnan(guard).all(), name + ": the guard row was written"
    assert not np.isnan(out).any(), name + ": an output was left unwritten (or is NaN)"
    assert form == r.FORM_OF_COUT[cout], (name, form)
    assert eng.fault_bits() == 0
    return out.reshape(-1, cout)


@pytest.mark.parametrize("name", sorted(r.GEOMS))
def test_conv_random_operands_with_the_epilogue(eng, name):
    cin, cout, rr, stride, h, w, n = r.GEOMS[name]
    kw, x, wt, want, bound = r.conv_case(name, 21)
    got = _conv(eng, name, x, wt, stride, **kw)
    _held(got, want, bound, name)
    if "relu" in kw:
        lo = kw.get("relu_from", 0)
        assert (got[:, lo:] >= 0).all() and (lo == 0 or (got[:, :lo] < 0).any())


@pytest.mark.parametrize("name", sorted(r.GEOMS))
def test_conv_exact_family_bit_for_bit(eng, name):
    cin, cout, rr, stride, h, w, n = r.GEOMS[name]
    x, wt = r.exact_operands(name, 11)
    acc, ab = r.conv_oracle(x, wt, stride)
    assert ab.max() < 2.0 ** 24 and np.abs(acc).max() > 8
    got = _conv(eng, name, x, wt, stride)                    # scale / shift NULL: 1 / 0
    diff = _bits16(got) != _bits16(acc.astype(np.float16))
    assert not diff.any(), "%s: %d of %d elements differ, first at %s" % (name, diff.sum(), diff.size, np.argwhere(diff)[0])


def test_conv_form_follows_the_geometry_only(eng):
    assert {r.FORM_OF_COUT[g[1]] for g in r.GEOMS.values()} == {1, 2}
    for name, want in (("l1", 1), ("l2d", 2)):
        x, wt = r.exact_operands(name, 11)
        assert eng.debug_any_conv_f16(x, wt, r.GEOMS[name][3])[2] == want
        assert eng.debug_any_conv_f16(x[:1], wt, r.GEOMS[name][3])[2] == want


@pytest.mark.parametrize("name", ["l2", "l1", "l2s"])
def test_conv_rows_have_the_same_bits_at_any_position_and_n(eng, name):
    """The same image alone, and as the 2nd of 3 (its rows then start inside a tile, not at row 0): bit-identical output rows."""
    cin, cout, rr, stride, h, w, n = r.GEOMS[name]
    x, wt, scale, shift, res = r.conv_operands(name, 31)
    three, _, _ = eng.debug_any_conv_f16(x, wt, stride, scale=scale, shift=shift)
    one, guard, _ = eng.debug_any_conv_f16(x[1:2], wt, stride, scale=scale, shift=shift)
    assert np.isnan(guard).all() and eng.fault_bits() == 0
    assert np.array_equal(_bits16(one[0]), _bits16(three[1]))
    assert not np.array_equal(_bits16(three[0]), _bits16(three[1]))


# ---------------------------------------------------------------------------------------------- 2. stem and max-pool
@pytest.mark.parametrize("size", r.STEM_SIZES, ids=["%dx%d" % s for s in r.STEM_SIZES])
def test_stem_and_pool(eng, size):
    h, w = size
    x, wt, scale, shift = r.stem_operands(h, w, 41)
    want, bound = r.stem_oracle(x, wt, scale, shift)
    stem, g1, pool, g2 = eng.debug_any_stem_f16(x, r.stem_pack16(wt), scale, shift)
    assert np.isnan(g1).all() and np.isnan(g2).all(), "a guard row was written"
    assert eng.fault_bits() == 0
    _held(stem, want, bound, "stem %dx%d" % size)
    assert not np.isnan(pool).any()
    want_pool = r.maxpool(stem.astype(np.float64)).astype(np.float16)
    assert pool.shape == want_pool.shape and np.array_equal(_bits16(pool), _bits16(want_pool)), "max-pool %dx%d" % size
    assert (r.maxpool(stem.astype(np.float64), 0.0) != want_pool).any()      # these maps tell a 0-padded pool apart


# ---------------------------------------------------------------------------------------------- 3. the tails
@pytest.mark.parametrize("c", r.TAIL_CS)
@pytest.mark.parametrize("hw", r.TAIL_HWS)
def test_norm_kernel(eng, hw, c):
    x, half, gamma, beta = r.norm_case(hw, c)
    want, bound = r.norm_oracle(x, gamma, beta, half)
    x2 = x.copy()
    x2[:, :, half:] = np.nan                                  # the BatchNorm half is the producer's: not touched
    got = eng.debug_any_norm_f16(x2, half, gamma, beta)
    assert np.isnan(got[x.size:]).all(), "the guard pixel was written"
    got = got[:x.size].reshape(x.shape)
    assert np.isnan(got[:, :, half:]).all(), "the BatchNorm half was touched"
    _held(got[:, :, :half], want, bound, "IBN finish, hw %d c %d" % (hw, c))
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("c", r.TAIL_CS)
@pytest.mark.parametrize("hw", r.TAIL_HWS)
def test_se_tail_kernel(eng, hw, c):
    y, sc, w1, w2t = r.se_case(hw, c)
    n = y.shape[0]
    want, gate, bound, gbound = r.se_oracle(y, sc, w1, w2t)
    out, g = eng.debug_any_se_tail_f16(y, sc, w1, w2t)
    assert np.isnan(out[y.size:]).all() and np.isnan(g[n * c:]).all(), "a guard pixel was written"
    _held(g[:n * c].reshape(n, c), gate, gbound, "SE gate, hw %d c %d" % (hw, c))
    _held(out[:y.size].reshape(y.shape), want, bound, "SE tail, hw %d c %d" % (hw, c))
    out2, g2 = eng.debug_any_se_tail_f16(y, sc, w1, w2t, alias=True)
    assert np.isnan(out2[y.size:]).all()
    assert np.array_equal(_bits16(out2[:y.size]), _bits16(out[:y.size])), "out aliasing y changed the bits"
    assert np.array_equal(_bits(g2[:n * c]), _bits(g[:n * c]))
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("p", [3.0, 2.6])
@pytest.mark.parametrize("c", r.TAIL_CS)
@pytest.mark.parametrize("hw", r.TAIL_HWS)
def test_gem_kernel(eng, hw, c, p):
    x, scale, shift = r.gem_case(hw, c)
    n = x.shape[0]
    g_want, e_want, gbound, ebound = anysize_ref.gem(x.astype(np.float64), p, scale, shift)
    g, e = eng.debug_any_gem_f16(x, p, scale, shift)
    assert np.isnan(g[n * c:]).all() and np.isnan(e[n * c:]).all(), "a guard pixel was written"
    _held(g[:n * c].reshape(n, c), g_want, gbound, "GeM, hw %d c %d p %g" % (hw, c, p))
    _held(e[:n * c].reshape(n, c), e_want, ebound, "BNNeck, hw %d c %d p %g" % (hw, c, p))
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 4. the forward
def _cos_err(a, b):
    return float((1.0 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)).max())


@pytest.mark.parametrize("k", r.FORWARD_CASES)
def test_forward_matches_reference_fixture(eng_w0, sd0, fx, k):
    eng = eng_w0
    p, h, w, n, seed, x = base._case_input(fx, k)
    xn = x.numpy()
    exact = eng.embed_f32_nchw(xn)
    eng.set_hw_precision(2)
    class3 = eng.embed_f32_nchw(xn)
    eng.set_hw_f16(True)                                      # hw_precision stays 2: the new setting wins
    eng.debug_keep(True)
    try:
        emb, logits = eng.embed_f32_nchw(xn, logits=True)
        taps = {}
        seres18.forward(sd0, x, taps)
        shapes = stage_shapes(h, w) + [(1, 1, 512)]
        worst = 0.0
        for s, name in enumerate(base.NAMES_ORACLE):
            t = taps[name]
            want = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1) if t.dim() == 4 else t.numpy().reshape(-1)
            got = eng.debug_stage(s, n, size=(h, w))
            assert got.size == n * int(np.prod(shapes[s])) == want.size, (s, got.size, want.size)
            err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
            print("stage %d (%s): rel max err %.3g against the oracle" % (s, name, err))
            assert err < r.STAGE_LIMIT, "stage %d (%s): rel max err %g" % (s, name, err)
            worst = max(worst, err)
    finally:
        eng.debug_keep(False)
    ce = _cos_err(emb, fx[p + "emb"])
    ee = np.abs(emb - fx[p + "emb"]).max() / np.abs(fx[p + "emb"]).max()
    le = np.abs(logits - fx[p + "logits"]).max() / np.abs(fx[p + "logits"]).max()
    print("(%d, %d): 1 - cos %.3g, emb %.3g, logits %.3g, worst stage %.3g" % (h, w, ce, ee, le, worst))
    assert ce < r.COS_LIMIT and ee < r.EMB_LIMIT and le < r.EMB_LIMIT
    assert np.array_equal(_bits(eng.embed_f32_nchw(xn)), _bits(emb))           # without the stage buffers: the same bits
    for flip, key in ((True, "desc_tta"), (False, "desc_plain")):
        got = eng.descriptor_f32_nchw(xn, flip_tta=flip)
        de = _cos_err(got, fx[p + key])
        print("%s: 1 - cos %.3g" % (key, de))
        assert got.shape == (n, 512 + 751) and de < r.COS_LIMIT
    assert not np.array_equal(_bits(emb), _bits(exact)), "hw_f16 returned the bits of hw_precision 0"
    assert not np.array_equal(_bits(emb), _bits(class3)), "hw_f16 returned the bits of hw_precision 2"


def test_generic_path_at_256x128_under_the_switch(eng_w0, golden_dir):
    """anysize_force sends (256, 128) through the new forward too: the fixture of the fixed-size forward under the same limits."""
    eng = eng_w0
    g = np.load(os.path.join(golden_dir, "seres18_seed0.npz"))
    x = seres18.preprocess_u8(synth.crops_u8(int(g["n"]), int(g["seed"]))).numpy()
    eng.set_hw_f16(True)
    plain = base._embed_hw(eng, x)[0]
    eng.debug_switch("anysize_force", 1)
    try:
        emb, logits = base._embed_hw(eng, x)
    finally:
        eng.debug_switch("anysize_force", 0)
    assert _cos_err(emb, g["emb"]) < r.COS_LIMIT
    assert np.abs(emb - g["emb"]).max() / np.abs(g["emb"]).max() < r.EMB_LIMIT
    assert np.abs(logits - g["logits"]).max() / np.abs(g["logits"]).max() < r.EMB_LIMIT
    assert not np.array_equal(_bits(emb), _bits(plain))


# ---------------------------------------------------------------------------------------------- 5. equalities, bit for bit
def test_results_do_not_depend_on_the_pass(eng_w0):
    eng = eng_w0
    eng.set_hw_f16(True)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 21, *SIZE)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    want_d = eng.descriptor_f32_nchw(x)
    parts = [eng.embed_f32_nchw(x[i:i + 1], logits=True) for i in range(3)]
    assert np.array_equal(_bits(np.concatenate([q[0] for q in parts])), _bits(want_e))
    assert np.array_equal(_bits(np.concatenate([q[1] for q in parts])), _bits(want_l))
    from reid_amd.engine import any_pass_size
    assert any_pass_size(1, *SIZE) > 3 > any_pass_size(1, 224, 268) == 1
    big = seres18.preprocess_u8(synth.smooth_crops_u8(3, 22, 224, 268)).numpy()
    want_b = eng.embed_f32_nchw(big)
    try:
        eng.set_chunk(1)                                       # (224, 268): a batch of 3 runs as 1 + 1 + 1
        assert np.array_equal(_bits(eng.embed_f32_nchw(big)), _bits(want_b))
        assert np.array_equal(_bits(eng.descriptor_f32_nchw(x)), _bits(want_d))
    finally:
        eng.set_chunk(1024)
    flipped = np.ascontiguousarray(x[:, :, :, ::-1])
    assert np.array_equal(_bits(eng.descriptor_f32_nchw(flipped, flip_tta=True)), _bits(want_d))
    assert not np.array_equal(_bits(eng.embed_f32_nchw(flipped)), _bits(want_e))


def test_host_and_device_entries_agree(eng_w0):
    eng = eng_w0
    eng.set_hw_f16(True)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(5, 22, *SIZE)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    want_d = eng.descriptor_f32_nchw(x)
    dx = DevArray.from_numpy(eng, x)
    de, dl, dd = DevArray(eng, (5, 512)), DevArray(eng, (5, 751)), DevArray(eng, (5, 1263))
    try:
        eng.embed_f32_nchw_dev(dx.ptr, 5, de.ptr, dl.ptr, size=SIZE)
        eng.descriptor_dev(dx.ptr, 5, True, dd.ptr, size=SIZE)
        eng.sync()
        assert np.array_equal(_bits(de.numpy()), _bits(want_e)) and np.array_equal(_bits(dl.numpy()), _bits(want_l))
        assert np.array_equal(_bits(dd.numpy()), _bits(want_d))
    finally:
        for a in (dx, de, dl, dd):
            a.free()


def test_uint8_entries_and_camera_indices(eng_w0):
    eng = eng_w0
    eng.set_hw_f16(True)
    images = [pil_resize_ref.formula_image(h, w, i) for i, (h, w) in enumerate(((90, 200), (64, 32), (257, 129), (90, 200)))]
    x = pil_resize_ref.preprocess(images, *SIZE)
    for flip in (True, False):
        want = eng.descriptor_f32_nchw(x, flip_tta=flip)
        assert np.array_equal(_bits(eng.descriptor_images_u8(images, flip_tta=flip, size=SIZE)), _bits(want))
    cams = np.asarray([2, 0, 5, 1], np.int32)
    eng.set_side_index(np.concatenate([cams, cams]))
    want = eng.descriptor_f32_nchw(x)
    eng.set_side_index(cams)
    got = eng.descriptor_images_u8(images, size=SIZE)
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(eng.descriptor_f32_nchw(x))), "the camera bias did not apply"


FRAME_H, FRAME_W = 120, 160
BOXES = np.array([[0, 0, 37, 51], [100, 60, 160, 120], [0, 80, 20, 120], [130, 0, 160, 9], [40, 30, 41, 31]], np.int32)


def test_frame_entries_equal_the_ragged_entry(eng_w0):
    """reid_embed_frame_u8_hw and reid_frame_submit_hw against reid_embed_ragged_u8_hw on the same pixels; a DeepSORT-sized pass is small
    enough for the fused fp32 front end, which hw_f16 must not take."""
    eng = eng_w0
    frame = np.random.default_rng(18).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    slices = [np.ascontiguousarray(frame[y1:y2, x1:x2]) for x1, y1, x2, y2 in BOXES]
    for size in ((128, 64), SIZE):
        eng.set_hw_f16(False)
        eng.set_hw_precision(0)
        exact = eng.embed_frame_u8(frame, BOXES, size=size)
        eng.set_hw_f16(True)
        want_e, want_l = eng.embed_ragged_u8(slices, size=size, logits=True)
        got_e, got_l = eng.embed_frame_u8(frame, BOXES, logits=True, size=size)
        assert np.array_equal(_bits(got_e), _bits(want_e)) and np.array_equal(_bits(got_l), _bits(want_l)), size
        assert not np.array_equal(_bits(got_e), _bits(exact)), size
        eng.frame_submit_hw(0, slices, size)
        eng.frame_cost(0, want_emb=True)
        emb, cost, iou = eng.frame_fetch(0)
        assert cost is None and iou is None and np.array_equal(_bits(emb), _bits(want_e)), size
    assert eng.embed_frame_u8(frame, BOXES[:0], size=SIZE).shape == (0, 512)


def test_camera_stream_equals_the_blocking_calls(eng_w0, blob0):
    from reid_amd.engine import Engine
    from reid_amd.iou_matching import iou_cost
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    from reid_amd.tracking import CameraStream
    import test_gpu_anysize_front as front
    pool = synth.ragged_crops_u8(9, seed=6)
    rng = np.random.default_rng(2)
    boxes = np.concatenate([rng.uniform(0, 200, (16, 2)), rng.uniform(10, 60, (16, 2))], 1)
    frames = front._frames(pool, 0)[:4]
    size, max_dist, budget = front.STREAM_SIZE, front.MAX_DIST, front.BUDGET
    log, tracks = [], []
    e = Engine(0)
    try:
        e.load_seres18(*blob0)
        e.set_hw_f16(True)
        met = NearestNeighborDistanceMetric("cosine", max_dist, budget, max_tracks=16, engine=e)
        for f, crops in enumerate(frames):
            feats = e.embed_ragged_u8(crops, size=size)
            cost = met.distance(feats, tracks, max_distance=max_dist) if tracks else None
            iou = iou_cost(boxes[:len(tracks)], boxes[:len(crops)]) if tracks else None
            rows, tg, after = front._plan(f, len(crops), tracks, 50)
            met.partial_fit(feats[rows], tg, after)
            log.append((feats, cost, iou, list(tracks), rows, tg, after))
            tracks = after
        met.close()
    finally:
        e.close()
    cam = CameraStream(*blob0, max_dist=max_dist, budget=budget, max_tracks=16, arch="seres18_hw", size=size, hw_f16=True)
    try:
        assert cam.eng.hw_f16 is True and cam.eng.hw_precision == -1
        cam.submit(frames[0])
        for f, (_, _, _, trk, rows, tg, after) in enumerate(log):
            got = cam.step(trk, boxes[:len(trk)], boxes[:len(frames[f])], frames[f + 1] if f + 1 < len(frames) else None)
            front._same(got, log[f], "CameraStream frame %d" % f)
            cam.commit(rows, tg, after)
        assert cam.eng.fault_bits() == 0
    finally:
        cam.close(destroy=True)
    eng_w0.set_hw_precision(0)
    assert not np.array_equal(_bits(eng_w0.embed_ragged_u8(frames[0], size=size)), _bits(log[0][0]))


# ---------------------------------------------------------------------------------------------- 6. the setting's rules
def test_the_setting(eng_w0, sd0, blob0):
    eng = eng_w0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 23, *SIZE)).numpy()
    big = seres18.preprocess_u8(synth.smooth_crops_u8(3, 24)).numpy()
    out = np.empty((3, 512), np.float32)

    def status(arr=x):
        return eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(arr), arr.shape[0], arr.shape[2], arr.shape[3], _p(out), None)

    # bad values: REID_ERR_ARG, nothing changes
    for bad in (2, -1, 7):
        assert eng.lib.reid_ctx_set_hw_f16(eng.h, bad) == -1 and "reid_ctx_set_hw_f16" in eng.lib.reid_last_error().decode()
    assert eng.lib.reid_ctx_set_hw_precision(eng.h, 1) == -1                # the pinned refusal of hw_precision 1 stays
    exact = eng.embed_f32_nchw(x)
    old = {}
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        old[mode] = eng.embed_f32_nchw(big)
    # default 0: today's refusal and message with the context in mode 1 / 2
    for mode in (1, 2):
        eng.set_precision(mode)
        assert status() == -1
        msg = eng.lib.reid_last_error().decode()
        assert "seres18_ibn" in msg and "mode %d" % mode in msg and "precision mode 0 (exact fp32) only" in msg
    # 1: runs whatever the mode and whatever hw_precision, always the same bits
    eng.set_hw_f16(True)
    seen = []
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        for v in (-1, 0, 2):
            eng.set_hw_precision(v)
            assert status() == 0, (mode, v, eng.lib.reid_last_error())
            seen.append(out.copy())
            assert eng.hw_precision == v
    assert all(np.array_equal(_bits(s), _bits(seen[0])) for s in seen) and not np.array_equal(_bits(seen[0]), _bits(exact))
    # (256, 128) is untouched in every mode
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        assert np.array_equal(_bits(eng.embed_f32_nchw(big)), _bits(old[mode])), mode
        assert status(big) == 0 and np.array_equal(_bits(out), _bits(old[mode])), mode
    # hw_precision governs again once hw_f16 is back at 0
    eng.set_precision(2)
    eng.set_hw_precision(0)
    eng.set_hw_f16(False)
    assert np.array_equal(_bits(eng.embed_f32_nchw(x)), _bits(exact))
    eng.set_hw_precision(-1)
    assert status() == -1 and "mode 2" in eng.lib.reid_last_error().decode()
    eng.set_precision(0)
    # the siblings are refused by name, whatever hw_siblings / hw_ema
    for arch, make in (("cares18_ibn", synth.cares18_state_dict), ("emares18_ibn", synth.emares18_state_dict)):
        eng.load_seres18(*weights.pack_seres18(make(0))[:2])
        try:
            for sib, ema in ((0, 0), (1, 1)):
                eng.set_hw_siblings(bool(sib))
                eng.set_hw_ema(bool(ema))
                eng.set_hw_f16(True)
                assert status() == -1
                msg = eng.lib.reid_last_error().decode()
                assert arch in msg and "fp16-storage any-size forward serves seres18_ibn only" in msg, msg
                assert status(big) == 0                                      # 256 x 128 runs them as before
                eng.set_hw_f16(False)
        finally:
            eng.set_hw_siblings(False)
            eng.set_hw_ema(False)
            eng.set_hw_f16(False)
            eng.load_seres18(*blob0)
    assert eng.fault_bits() == 0


def test_refusals_come_before_the_slot_is_touched(eng_w0, blob0):
    eng = eng_w0
    crops, size = synth.ragged_crops_u8(3, seed=6), (128, 64)
    eng.set_hw_f16(True)
    want = eng.embed_ragged_u8(crops, size=size)
    eng.frame_submit_hw(1, crops, size)
    eng.frame_cost(1, want_emb=True)
    eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
    try:
        eng.set_hw_siblings(True)
        slab, offs, hw, n = eng._frame_pack(1, crops)
        assert eng.lib.reid_frame_submit_hw(eng.h, 1, _p(slab), _p(offs), _p(hw), n, size[0], size[1], None) == -1
        msg = eng.lib.reid_last_error().decode()
        assert "cares18_ibn" in msg and "serves seres18_ibn only" in msg, msg
        assert np.array_equal(_bits(eng.frame_fetch(1)[0]), _bits(want)), "a refused submit touched the pending frame"
    finally:
        eng.set_hw_siblings(False)
        eng.load_seres18(*blob0)


def test_plugin_objects(eng_w0, sd0, fx):
    from reid_amd import inference_utils, reid_inference
    from reid_amd.backbone import seres18_ibn
    from reid_amd.extractor import Extractor
    eng = eng_w0
    p, h, w, n, seed, x = base._case_input(fx, 1)
    crops = synth.ragged_crops_u8(4, seed=5)
    eng.set_hw_f16(True)
    want = eng.embed_f32_nchw(x.numpy())
    want_crops = eng.embed_ragged_u8(crops, size=(h, w))
    want_desc = eng.descriptor_f32_nchw(x.numpy())
    eng.set_hw_f16(False)
    model = seres18_ibn(num_classes=751, loss="triplet", hw_f16=True)
    model.load_state_dict(sd0)
    for mode in (0, 2):
        eng.set_precision(mode)
        got = np.asarray(model(x.numpy()))
        assert eng.precision == mode and eng.hw_f16 is False and eng.hw_precision == -1      # the engine's settings came back
        assert np.array_equal(_bits(got), _bits(want))
    eng.set_precision(0)
    ext = Extractor(sd0, size=(w, h), hw_f16=True)
    assert ext.size == (w, h)
    feats = ext(crops)
    assert eng.hw_f16 is False and eng.hw_precision == -1
    assert np.array_equal(_bits(feats), _bits(want_crops))
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    assert np.array_equal(_bits(inference_utils.extract_descriptors(x.numpy(), hw_f16=True)), _bits(want_desc))
    assert eng.hw_f16 is False
    d = DevArray(eng, (n, 1263))
    try:
        reid_inference.inference_efficient(eng, x.numpy(), d.ptr, arch="seres18_hw", hw_f16=True)
        assert np.array_equal(_bits(d.numpy()), _bits(want_desc)) and eng.hw_f16 is False
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------- 7. without the library
_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
x = np.zeros((1, 3, 96, 72), np.float32)
eng.set_hw_precision(0)
before = eng.embed_f32_nchw(x)
eng.set_hw_f16(True)
try:
    eng.embed_f32_nchw(x)
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_anysize_f16.so" in str(e)
    eng.set_hw_f16(False)
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.embed_f32_nchw(x), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_anysize_f16.so, loaded through REID_HIP_LIB in a fresh child process: hw_f16 1 at another
    size is REID_ERR_STATE naming the file before anything is launched, and hw_precision 0 works before and after it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_anysize_f16.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    res = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "RAISED -3" in res.stdout and lib in res.stdout
