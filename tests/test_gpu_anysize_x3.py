"""ResNet18-IBN-SE at any input size in the fp32-class arithmetic on the MI355X (pytest -m gpu tests/test_gpu_anysize_x3.py).

Kernel: any_conv_x3_kernel (libreid_hip_anysize_x3.so) through reid_debug_any_conv, the launcher the forward calls, on the geometries of
tests/anysize_x3_ref.py - the smallest shapes at which each code path can go wrong.
  * exact family: the output equals the numpy restatement's fp32 value BIT FOR BIT (tests/test_anysize_x3_host.py shows why fp32
    accumulation is exact there, and that a dropped product changes 86-98 % of the outputs);
  * random operands with the epilogue on, and the small family (f16 subnormals in both parts): every element within the bound
    tests/test_gpu_conv.py derives for the split arithmetic (SAFETY = 2) of the float64 oracle;
  * hw_precision 0 on the same operands is within its own bound and has other bits (the route is real); each tile form is reached; an
    image's rows do not depend on its position in the batch.
Every output has a guard row that must still read as NaN, and the fault status is 0.

Forward: reid_ctx_set_hw_precision(2) on the seres18_seed0 weights under the limits tests/test_gpu_anysize.py applies to mode 0 (the
project's rule that the fp32-class arithmetic meets mode 0's bar), within 2e-5 of mode 0's embeddings (DESIGN's figure for mode 2
against mode 0) with other bits, the equalities of that module bit for bit, the setting's rules, the plugin objects, and a build without
the side library."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import matching, seres18
from reid_amd import _ffi, synth, weights
from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_x3_ref as x3  # noqa: E402
import pil_resize_ref  # noqa: E402
import test_gpu_anysize as base  # noqa: E402
from test_gpu_conv import bound, conv_oracle, epilogue  # noqa: E402

pytestmark = [pytest.mark.gpu]

EMB_LIMIT, DESC_LIMIT = base.EMB_LIMIT, base.DESC_LIMIT      # with STAGE_LIMIT and COS_LIMIT inside base._check_forward: mode 0's limits
MODE0_LIMIT = 2e-5                       # mode 2 against mode 0, relative to the largest magnitude
FORM_OF_COUT = {64: 1, 128: 2, 256: 2, 512: 2}          # anysize_x3.h: 128 x 64 tiles for 64 output channels, 128 x 128 above
RES_RELU = ("l1big", "l2", "l3", "l4")
RELU_FROM_HALF = ("l1", "l2s")
_bits, _p = base._bits, base._p


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    yield e
    e.clear_fault()
    e.debug_switch("anysize_force", 0)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anysize.npz"))


@pytest.fixture(scope="module")
def sd0():
    return synth.seres18_state_dict(0)


@pytest.fixture()
def eng_w0(eng, sd0):
    eng.set_precision(0)
    eng.set_hw_precision(-1)
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    yield eng
    eng.set_precision(0)
    eng.set_hw_precision(-1)
    assert eng.fault_bits() == 0


def _conv(eng, name, x, wt, hw_precision=2, **kw):
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    out, guard, form = eng.debug_any_conv(x, wt, stride, hw_precision=hw_precision, **kw)
    assert np.isnan(guard).all(), name + ": the guard row was written"
    assert not np.isnan(out).any(), name + ": an output was left unwritten (or is NaN)"
    assert form == (FORM_OF_COUT[cout] if hw_precision == 2 else 0), (name, form)
    assert eng.fault_bits() == 0
    return out.reshape(-1, cout)


def _held(got, want, b, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / b).max())
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), worst))
    assert (err <= b).all(), "%s: err / bound %.3g" % (what, worst)


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("name", sorted(x3.GEOMS))
def test_exact_family_bit_for_bit(eng, name):
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    x, wt = x3.exact_operands(name, 11)
    val, mag = x3.restate(x, wt, stride)
    assert mag.max() / 0.25 < 2.0 ** 24
    got = _conv(eng, name, x, wt, scale=np.ones(cout, np.float32), shift=np.zeros(cout, np.float32))
    want = val.astype(np.float32)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s" % (name, diff.sum(), diff.size, np.argwhere(diff)[0])


@pytest.mark.parametrize("name", sorted(x3.GEOMS))
def test_random_operands_with_the_epilogue(eng, name):
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    x, wt, scale, shift, res = x3.random_operands(name, 21)
    k = r * r * cin
    kw = dict(scale=scale, shift=shift)
    if name in RES_RELU:
        kw.update(res=res, relu=True)
    elif name in RELU_FROM_HALF:
        kw.update(relu=True, relu_from=cout // 2)
    ho, wo = x3.out_hw(name)
    acc, ab = conv_oracle(x, wt, stride, x3.pad_of(r), np.arange(n * ho * wo))
    rr = res.reshape(-1, cout).astype(np.float64) if "res" in kw else None
    want = epilogue(acc, scale, shift, rr, kw.get("relu", False), kw.get("relu_from", 0))
    got2 = _conv(eng, name, x, wt, **kw)
    _held(got2, want, bound(acc, ab, wt, k, True, scale, shift, rr), name + " fp32-class")
    got0 = _conv(eng, name, x, wt, hw_precision=0, **kw)
    _held(got0, want, bound(acc, ab, wt, k, False, scale, shift, rr), name + " exact fp32")
    assert not np.array_equal(_bits(got0), _bits(got2)), name + ": hw_precision 2 returned the exact-fp32 bits"
    if "relu" in kw:
        lo = kw.get("relu_from", 0)
        assert (got2[:, lo:] >= 0).all() and (lo == 0 or (got2[:, :lo] < 0).any())


@pytest.mark.parametrize("name", ("l2d", "l1", "l4"))
def test_small_family_keeps_f16_subnormals(eng, name):
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    x, wt = x3.small_operands(name, 12)
    ho, wo = x3.out_hw(name)
    acc, ab = conv_oracle(x, wt, stride, x3.pad_of(r), np.arange(n * ho * wo))
    got = _conv(eng, name, x, wt, scale=np.ones(cout, np.float32), shift=np.zeros(cout, np.float32))
    _held(got, acc, bound(acc, ab, wt, r * r * cin, True), name + " small family")


def test_every_tile_form_is_reached(eng):
    """Both tile forms are among the geometries (_conv asserts form_out of every launch), and the form follows the geometry, not n."""
    assert {FORM_OF_COUT[g[1]] for g in x3.GEOMS.values()} == {1, 2}
    for name, want in (("l1", 1), ("l2d", 2)):
        x, wt = x3.exact_operands(name, 11)
        assert eng.debug_any_conv(x, wt, x3.GEOMS[name][3])[2] == want
        assert eng.debug_any_conv(x[:1], wt, x3.GEOMS[name][3])[2] == want


def test_rows_do_not_depend_on_the_image_position(eng):
    """l2: the same image alone, and as the 2nd of 3 (its rows then start at row 20 of a tile, not 0): bit-identical output rows."""
    cin, cout, r, stride, h, w, n = x3.GEOMS["l2"]
    x, wt, scale, shift, res = x3.random_operands("l2", 31)
    three, _, _ = eng.debug_any_conv(x, wt, stride, scale=scale, shift=shift)
    one, guard, _ = eng.debug_any_conv(x[1:2], wt, stride, scale=scale, shift=shift)
    assert np.isnan(guard).all() and eng.fault_bits() == 0
    assert np.array_equal(_bits(one[0]), _bits(three[1]))
    assert not np.array_equal(_bits(three[0]), _bits(three[1]))


# ---------------------------------------------------------------------------------------------- 2. the forward
@pytest.mark.parametrize("k", [0, 1, 2])
def test_forward_matches_reference_fixture(eng_w0, sd0, fx, k):
    eng = eng_w0
    p, h, w, n, seed, x = base._case_input(fx, k)
    exact = eng.embed_f32_nchw(x.numpy())
    eng.set_hw_precision(2)
    taps = {name: fx[p + "tap_" + name] for name in base.NAMES_REF}
    emb, logits = base._check_forward(eng, sd0, x, fx[p + "emb"], fx[p + "logits"], taps, lambda a: eng.embed_f32_nchw(a, logits=True))
    assert np.array_equal(_bits(eng.embed_f32_nchw(x.numpy())), _bits(emb))
    for flip, key in ((True, "desc_tta"), (False, "desc_plain")):
        got = eng.descriptor_f32_nchw(x.numpy(), flip_tta=flip)
        err = np.abs(got - fx[p + key]).max()
        print("%s: max |err| %.3g" % (key, err))
        assert got.shape == (n, 512 + 751) and err <= DESC_LIMIT
    assert not np.array_equal(_bits(emb), _bits(exact)), "hw_precision 2 returned the exact-fp32 bits"
    rel = np.abs(emb - exact).max() / np.abs(exact).max()
    print("against hw_precision 0: rel max diff %.3g" % rel)
    assert rel < MODE0_LIMIT


def test_generic_path_at_256x128(eng_w0, sd0, golden_dir):
    eng = eng_w0
    g = np.load(os.path.join(golden_dir, "seres18_seed0.npz"))
    x = seres18.preprocess_u8(synth.crops_u8(int(g["n"]), int(g["seed"])))
    taps = {name: g["tap_" + name] for name in base.NAMES_REF}
    eng.debug_switch("anysize_force", 1)
    try:
        exact = base._embed_hw(eng, x.numpy())[0]
        eng.set_hw_precision(2)
        emb, logits = base._check_forward(eng, sd0, x, g["emb"], g["logits"], taps, lambda a: base._embed_hw(eng, a))
        assert not np.array_equal(_bits(emb), _bits(exact))
        assert np.abs(emb - exact).max() / np.abs(exact).max() < MODE0_LIMIT
    finally:
        eng.debug_switch("anysize_force", 0)


def test_results_do_not_depend_on_the_pass(eng_w0):
    eng = eng_w0
    eng.set_hw_precision(2)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(7, 21, 96, 72)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    want_d = eng.descriptor_f32_nchw(x)
    for m in (1, 2, 5):
        parts = [eng.embed_f32_nchw(x[i:i + m], logits=True) for i in range(0, 7, m)]
        assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(want_e)), m
        assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(want_l)), m
        assert np.array_equal(_bits(np.concatenate([eng.descriptor_f32_nchw(x[i:i + m]) for i in range(0, 7, m)])), _bits(want_d)), m
    try:
        for chunk in (1, 2):
            eng.set_chunk(chunk)
            e, l = eng.embed_f32_nchw(x, logits=True)
            assert np.array_equal(_bits(e), _bits(want_e)) and np.array_equal(_bits(l), _bits(want_l)), chunk
            assert np.array_equal(_bits(eng.descriptor_f32_nchw(x)), _bits(want_d)), chunk
    finally:
        eng.set_chunk(1024)
    # the flip-TTA descriptor of a mirrored batch is the descriptor of the batch
    flipped = np.ascontiguousarray(x[:, :, :, ::-1])
    assert np.array_equal(_bits(eng.descriptor_f32_nchw(flipped, flip_tta=True)), _bits(want_d))
    assert not np.array_equal(_bits(eng.embed_f32_nchw(flipped)), _bits(want_e))


def test_host_and_device_entries_agree(eng_w0):
    eng = eng_w0
    eng.set_hw_precision(2)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(5, 22, 96, 72)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    want_d = eng.descriptor_f32_nchw(x)
    dx = DevArray.from_numpy(eng, x)
    de, dl, dd = DevArray(eng, (5, 512)), DevArray(eng, (5, 751)), DevArray(eng, (5, 1263))
    try:
        eng.embed_f32_nchw_dev(dx.ptr, 5, de.ptr, dl.ptr, size=(96, 72))
        eng.descriptor_dev(dx.ptr, 5, True, dd.ptr, size=(96, 72))
        eng.sync()
        assert np.array_equal(_bits(de.numpy()), _bits(want_e)) and np.array_equal(_bits(dl.numpy()), _bits(want_l))
        assert np.array_equal(_bits(dd.numpy()), _bits(want_d))
    finally:
        for a in (dx, de, dl, dd):
            a.free()


def test_uint8_entries_and_camera_indices(eng_w0, sd0):
    eng = eng_w0
    eng.set_hw_precision(2)
    images = [pil_resize_ref.formula_image(h, w, i) for i, (h, w) in enumerate(((90, 200), (64, 32), (257, 129), (90, 200)))]
    x = pil_resize_ref.preprocess(images, 96, 72)
    for flip in (True, False):
        want = eng.descriptor_f32_nchw(x, flip_tta=flip)
        assert np.array_equal(_bits(eng.descriptor_images_u8(images, flip_tta=flip, size=(96, 72))), _bits(want))
    cams = np.asarray([2, 0, 5, 1], np.int32)
    eng.set_side_index(np.concatenate([cams, cams]))
    want = eng.descriptor_f32_nchw(x)
    eng.set_side_index(cams)
    got = eng.descriptor_images_u8(images, size=(96, 72))
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(eng.descriptor_f32_nchw(x))), "the camera bias did not apply"
    # the cv2-style entry against the float entry on the same crops preprocessed on the host (the limit of the extractor test of mode 0)
    crops = synth.ragged_crops_u8(4, seed=5)
    feats = eng.embed_ragged_u8(crops, size=(96, 72))
    host = eng.embed_f32_nchw(matching.preprocess(crops, size=(72, 96)))
    assert np.abs(feats - host).max() / np.abs(host).max() < EMB_LIMIT


def test_the_setting(eng_w0, sd0):
    eng = eng_w0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 23, 96, 72)).numpy()
    big = seres18.preprocess_u8(synth.smooth_crops_u8(3, 24)).numpy()
    out = np.empty((3, 512), np.float32)

    def status(arr=x):
        return eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(arr), arr.shape[0], arr.shape[2], arr.shape[3], _p(out), None)

    for bad in (1, 3, -2):
        assert eng.lib.reid_ctx_set_hw_precision(eng.h, bad) == -1 and "reid_ctx_set_hw_precision" in eng.lib.reid_last_error().decode()
    assert eng.hw_precision == -1
    exact = eng.embed_f32_nchw(x)
    old = {}
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        old[mode] = eng.embed_f32_nchw(big)
    # -1: today's rule
    eng.set_precision(2)
    assert status() == -1
    msg = eng.lib.reid_last_error().decode()
    assert "seres18_ibn" in msg and "mode 2" in msg
    # 0 with the context in mode 2: runs, mode 0's bits
    eng.set_hw_precision(0)
    assert np.array_equal(_bits(eng.embed_f32_nchw(x)), _bits(exact))
    # 2 with the context in mode 2 and in mode 0: the same bits, not mode 0's
    eng.set_hw_precision(2)
    in2 = eng.embed_f32_nchw(x)
    eng.set_precision(0)
    assert np.array_equal(_bits(eng.embed_f32_nchw(x)), _bits(in2)) and not np.array_equal(_bits(in2), _bits(exact))
    # 256 x 128 is not affected by the setting, in any mode
    for v in (-1, 0, 2):
        eng.set_hw_precision(v)
        for mode in (0, 1, 2):
            eng.set_precision(mode)
            assert np.array_equal(_bits(eng.embed_f32_nchw(big)), _bits(old[mode])), (v, mode)
            assert status(big) == 0 and np.array_equal(_bits(out), _bits(old[mode])), (v, mode)
    eng.set_precision(0)
    # the siblings stay refused at other sizes whatever the setting
    eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
    try:
        for v in (-1, 0, 2):
            eng.set_hw_precision(v)
            assert status() == -1 and "cares18_ibn" in eng.lib.reid_last_error().decode(), v
    finally:
        eng.set_hw_precision(-1)
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])


def test_weights_it_cannot_split_are_refused(eng_w0, sd0):
    from reid_amd._ffi import ReidHipError
    eng = eng_w0
    sd = synth.seres18_state_dict(0)
    sd["basicBlock31.block_pre.conv2.weight"] = np.array(sd["basicBlock31.block_pre.conv2.weight"], copy=True)
    sd["basicBlock31.block_pre.conv2.weight"][3, 5, 1, 1] = 40.0
    blob, manifest, _ = weights.pack_seres18(sd)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(2, 25, 64, 32)).numpy()
    try:
        eng.load_seres18(blob, manifest)
        with pytest.raises(ReidHipError, match=r"b31\.conv2\.w") as ei:
            eng.set_hw_precision(2)
        assert ei.value.status == -1 and eng.hw_precision == -1
        eng.set_hw_precision(0)
        assert np.isfinite(eng.embed_f32_nchw(x)).all()
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])
        eng.set_hw_precision(2)
        with pytest.raises(ReidHipError, match=r"b31\.conv2\.w") as ei:
            eng.load_seres18(blob, manifest)
        assert ei.value.status == -1
        assert np.isfinite(eng.embed_f32_nchw(x)).all()                     # the good checkpoint is still the loaded one
    finally:
        eng.set_hw_precision(-1)
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])


def test_activation_overflow_raises_the_fault_word(eng_w0, sd0):
    """A stem BatchNorm scaled by 1e7 at (64, 32): the loader of the first trunk convolution meets values f16 cannot hold and raises bit 0
    of the library's status word - REID_ERR_STATE until clear_fault; hw_precision 0 runs the same checkpoint."""
    from reid_amd._ffi import ReidHipError
    eng = eng_w0
    sd = synth.seres18_state_dict(0)
    sd["bn0.weight"] = np.asarray(sd["bn0.weight"]) * 1e7
    x = seres18.preprocess_u8(synth.smooth_crops_u8(2, 26, 64, 32)).numpy()
    try:
        eng.load_seres18(*weights.pack_seres18(sd)[:2])
        assert np.isfinite(eng.embed_f32_nchw(x)).all()
        eng.set_hw_precision(2)
        with pytest.raises(ReidHipError, match="outside f16's range") as ei:
            eng.embed_f32_nchw(x)
        assert ei.value.status == -3 and eng.fault_bits() & 1
        with pytest.raises(ReidHipError, match="outside f16's range"):
            eng.embed_f32_nchw(x)                                           # sticky
        eng.clear_fault()
        assert eng.fault_bits() == 0
        eng.set_hw_precision(0)
        assert np.isfinite(eng.embed_f32_nchw(x)).all()
    finally:
        eng.clear_fault()
        eng.set_hw_precision(-1)
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])


def test_plugin_objects(eng_w0, sd0, fx):
    from reid_amd import reid_inference
    from reid_amd.backbone import seres18_ibn
    from reid_amd.extractor import Extractor
    eng = eng_w0
    p, h, w, n, seed, x = base._case_input(fx, 1)
    crops = synth.ragged_crops_u8(4, seed=5)
    eng.set_hw_precision(2)
    want = eng.embed_f32_nchw(x.numpy())
    want_crops = eng.embed_ragged_u8(crops, size=(96, 72))
    eng.set_hw_precision(-1)
    exact = eng.embed_f32_nchw(x.numpy())
    model = seres18_ibn(num_classes=751, loss="triplet", hw_precision="f16x3")
    model.load_state_dict(sd0)
    for mode in (0, 2):
        eng.set_precision(mode)
        got = np.asarray(model(x.numpy()))
        assert eng.precision == mode and eng.hw_precision == -1             # the engine's settings came back
        assert np.array_equal(_bits(got), _bits(want))
    eng.set_precision(0)
    plain = seres18_ibn(num_classes=751, loss="triplet")
    plain.load_state_dict(sd0)
    assert np.array_equal(_bits(np.asarray(plain(x.numpy()))), _bits(exact))   # None keeps exact fp32 for such a call
    ext = Extractor(sd0, size=(72, 96), precision="f16x3")
    assert ext.size == (72, 96) and ext.precision == "f16x3"
    feats = ext(crops)
    assert eng.precision == 0 and eng.hw_precision == -1
    assert np.array_equal(_bits(feats), _bits(want_crops))
    # the evaluation chain at the VeRi geometry: its descriptors are the engine's at hw_precision 2
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    rng = np.random.default_rng(100)
    gl, gc, gs = rng.integers(0, 4, 12), np.arange(12) % 2, rng.integers(0, 3, 12)
    ql, qc, qs = rng.integers(1, 4, 4), np.arange(4) % 2, rng.integers(0, 3, 4)
    gx = synth.identity_images_f32(gl, gc, 101, h=224, w=268)
    qx = synth.identity_images_f32(ql, qc, 102, h=224, w=268)
    taps = {}
    cmc, m_ap = reid_inference.evaluate_reid(gx, gl, gc, gs, qx, ql, qc, qs, engine=eng, arch="seres18_hw", taps=taps, verbose=False, k1=6, k2=3,
                                             cluster_fn=lambda d: np.zeros(d.shape[0], np.int64), hw_precision="f16x3")
    assert cmc.shape == (12,) and 0.0 <= m_ap <= 1.0 and eng.hw_precision == -1
    eng.set_hw_precision(2)
    assert np.array_equal(_bits(taps["desc"][:12]), _bits(eng.descriptor_f32_nchw(gx)))
    eng.set_hw_precision(0)
    assert not np.array_equal(_bits(taps["desc"][:12]), _bits(eng.descriptor_f32_nchw(gx)))


def test_a_checkpoint_outside_the_range_falls_back_with_one_log_line(eng_w0, sd0, caplog):
    from reid_amd.backbone import seres18_ibn
    eng = eng_w0
    sd = synth.seres18_state_dict(0)
    sd["basicBlock31.block_pre.conv2.weight"] = np.array(sd["basicBlock31.block_pre.conv2.weight"], copy=True)
    sd["basicBlock31.block_pre.conv2.weight"][3, 5, 1, 1] = 40.0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(2, 27, 64, 32)).numpy()
    model = seres18_ibn(num_classes=751, loss="triplet", precision="f32", hw_precision="f16x3")
    model.load_state_dict(sd)
    try:
        with caplog.at_level("WARNING", logger="root.tracker"):
            a = np.asarray(model(x))
            b = np.asarray(model(x))
        assert len([r for r in caplog.records if "fp32-class" in r.getMessage()]) == 1
        eng.set_hw_precision(0)
        assert np.array_equal(_bits(a), _bits(eng.embed_f32_nchw(x))) and np.array_equal(_bits(a), _bits(b))
    finally:
        eng.set_hw_precision(-1)
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])


# ---------------------------------------------------------------------------------------------- 3. without the library
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
eng.set_hw_precision(2)
try:
    eng.embed_f32_nchw(x)
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_anysize_x3.so" in str(e)
    eng.set_hw_precision(0)
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.embed_f32_nchw(x), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_anysize_x3.so, loaded through REID_HIP_LIB in a fresh child process: hw_precision 2 at
    another size is REID_ERR_STATE naming the file before anything is launched, and hw_precision 0 works before and after it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_anysize_x3.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED -3" in r.stdout and lib in r.stdout
