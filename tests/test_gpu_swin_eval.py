"""The Swin side of the evaluation chain on the MI355X (pytest -m gpu): the three kernels of libreid_hip_swin_eval.so alone, the
descriptor entry points composed from them, and the result against the reference's own swin_t (tests/golden/swin_eval.npz, made by
tools/gen_golden_swin_eval.py).

The synthetic Swin is almost flip-invariant - the fixture's TTA descriptor differs from the normalised plain-view one by 1.9e-3 - so a
bar against the reference alone could pass a build that forgets to mirror.  The mirror is therefore proved exactly (tests 1 and 2:
bit-equality with the plain stem on a host-flipped input) and by the composition test (4), whose bound is the descriptor kernel's own
(tests/swin_eval_ref.py holds the float64 restatement and the derivation) and is asserted to be more than 100 times smaller than the
TTA effect; the bar against the reference (5) is tied to the stored effect sizes."""
import os
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_crops_ref as cref  # noqa: E402
import swin_eval_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

VIEWS = 6
SIZE = (448, 224)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.set_side_index(None)
    e.set_precision(0)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "swin_eval.npz"))


@pytest.fixture(scope="module")
def sds():
    """The fixture's weights: 751 classes, a side table of 6 views, both versions."""
    return {v: synth.swin_state_dict(0, views=VIEWS, version=v) for v in ("v1", "v2")}


@pytest.fixture(scope="module")
def blobs(sds):
    out = {v: weights.pack_swin(sd)[:2] for v, sd in sds.items()}
    out["nocls"] = weights.pack_swin({k: v for k, v in sds["v1"].items() if not k.startswith("mlp_head")})[:2]
    return out


@pytest.fixture(scope="module")
def x5():
    return synth.images_f32(5, 5, h=SIZE[0], w=SIZE[1])


def _load(eng, blobs, key, mode, chunk=1024):
    eng.set_side_index(None)
    eng.set_precision(0)
    eng.load_swin(*blobs[key])
    eng.set_precision(mode)
    eng.set_chunk(chunk)


def _flip(x):
    return np.ascontiguousarray(x[..., ::-1])


# ----------------------------------------------------------------------------- 1. sfe_conv1_mirror_kernel
@pytest.mark.parametrize("hw", [(224, 224), (448, 224)], ids=["224x224", "448x224"])
def test_conv1_mirror_is_conv1_of_the_flipped_image(eng, hw):
    """Bit-equal to sfe_conv1_kernel on the host-flipped input, n = 3 (several blocks); and not the plain stem's result."""
    w, b = cref.conv_weights()
    x = synth.images_f32(3, 21, h=hw[0], w=hw[1])
    eng.set_precision(0)
    got = eng.debug_swin_conv1(x, w, b, mirror=True)
    assert got.shape == (3, hw[0] // 2, hw[1] // 2, 12) and np.isfinite(got).all()          # NaN fill: every element written
    np.testing.assert_array_equal(got, eng.debug_swin_conv1(_flip(x), w, b))
    assert not np.array_equal(got, eng.debug_swin_conv1(x, w, b))


# ----------------------------------------------------------------------------- 2. swin_crop_front_mirror_kernel
@pytest.mark.parametrize("size", [(224, 224), (448, 224)], ids=["224x224", "448x224"])
def test_crop_front_mirror_is_conv1_of_the_resized_then_flipped_crops(eng, size):
    """Packed crops and windows of a frame (pitch 640) give the same bits: those of sfe_conv1_kernel on the crops resized, normalised and
    THEN flipped on the host.  The crop set holds 1-pixel-wide and 1-pixel-high crops, odd and even widths, the identity, crops scaled up
    and scaled down; mean / std are not ImageNet's."""
    frame, crops, _ = cref.crop_set()
    ms = cref.OTHER_MEAN_STD
    w, b = cref.conv_weights()
    eng.set_precision(0)
    pk, offsets, hw = cref.packed(crops)
    assert {c.shape[1] % 2 for c in crops} == {0, 1} and any(c.shape[1] == 1 for c in crops)
    assert any(c.shape[0] < size[0] and c.shape[1] < size[1] for c in crops) and any(c.shape[0] > size[0] and c.shape[1] > size[1] for c in crops)
    got = eng.debug_swin_crop_front(pk, offsets, hw, w, b, size=size, mean_std=ms, mirror=True)
    assert got.shape == (len(crops), size[0] // 2, size[1] // 2, 12) and np.isfinite(got).all()
    f_off = np.array([(y * cref.FRAME_W + x) * 3 for y, x in cref.CROP_YX], np.int64)
    from_frame = eng.debug_swin_crop_front(frame, f_off, hw, w, b, size=size, mean_std=ms, pitch=cref.FRAME_W, mirror=True)
    np.testing.assert_array_equal(from_frame, got, err_msg="windows of a frame against packed crops")
    pre = cref.preprocess(crops, size, ms[:3], ms[3:])
    np.testing.assert_array_equal(got, eng.debug_swin_conv1(_flip(pre), w, b), err_msg="resize -> normalise -> flip -> sfe_conv1_kernel")
    # mirroring the source crop first is a different image wherever the resize resamples (half-pixel centres are symmetric, fp32 taps are not)
    assert not np.array_equal(got, eng.debug_swin_crop_front(pk, offsets, hw, w, b, size=size, mean_std=ms))


# ----------------------------------------------------------------------------- 3. swin_descriptor_kernel
def _desc_operands(n, nc, seed):
    rng = np.random.default_rng(seed)
    e1 = rng.normal(0, 1.0, (n, 96)).astype(np.float32)
    e2 = (e1 + rng.normal(0, 0.05, (n, 96))).astype(np.float32)              # a mirrored view: close to the plain one
    w = rng.normal(0, 0.1, (nc, 96)).astype(np.float32)
    return e1, e2, w


@pytest.mark.parametrize("tta", [True, False], ids=["tta", "plain"])
@pytest.mark.parametrize("nc", [751, 5, 1])
def test_descriptor_kernel_against_float64(eng, nc, tta):
    """n = 4 rows, row 2 all zero in both views, into a [6][nc + 96 + 3] NaN-filled output: every owned element within the derived bound
    (tests/swin_eval_ref.py) of float64, the zero row zero, the two extra rows and three extra columns still NaN."""
    e1, e2, w = _desc_operands(4, nc, 30 + nc)
    e1[2] = 0.0
    e2[2] = 0.0
    d = nc + 96
    eng.set_precision(0)
    out = eng.debug_swin_descriptor(e1, e2 if tta else None, w, out_rows=6, ld=d + 3)
    got = out[:4, :d]
    assert np.isnan(out[4:]).all() and np.isnan(out[:, d:]).all(), "the launch wrote outside its rows / columns"
    assert np.isfinite(got).all() and (got[2] == 0).all()
    want, bound = ref.descriptor64(e1, e2 if tta else None, w)
    err = np.abs(got.astype(np.float64) - want)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max())
    print("RATIO swin_descriptor nc=%d tta=%d worst err/bound %.4f (largest bound %.2e)" % (nc, tta, ratio, bound.max()))
    assert (err <= bound).all(), "worst err/bound %.3f" % ratio
    assert ratio > 0.0
    nrm = np.linalg.norm(got.astype(np.float64), axis=1)
    np.testing.assert_allclose(np.delete(nrm, 2), 1.0 if tta else np.sqrt(2.0), atol=1e-6)       # one view: two unit vectors, not renormalised
    # the logits part comes first
    np.testing.assert_allclose(np.linalg.norm(got[[0, 1, 3], :nc].astype(np.float64), axis=1), np.sqrt(0.5) if tta else 1.0, atol=2e-2 if tta else 1e-6)


def test_descriptor_kernel_single_row(eng):
    e1, e2, w = _desc_operands(1, 751, 77)
    eng.set_precision(0)
    got = eng.debug_swin_descriptor(e1, e2, w)
    want, bound = ref.descriptor64(e1, e2, w)
    assert got.shape == (1, 847) and (np.abs(got.astype(np.float64) - want) <= bound).all()


# ----------------------------------------------------------------------------- 4. composition
@pytest.mark.parametrize("side", [False, True], ids=["noside", "side"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_descriptor_entry_is_the_kernel_on_the_two_embeddings(eng, fx, sds, blobs, x5, version, mode, side):
    """reid_swin_descriptor_f32_nchw (5 images at 448 x 224 in passes of 2, 2, 1) against the float64 oracle of test 3 fed with what
    reid_swin_embed_f32_nchw returns for x and for the host-flipped x (with the same side indices), held to test 3's bound: this isolates
    the new code - the mirrored stem, the passes, the side indices handed to both views, the order of the parts - from the forward.  The
    fixture's TTA effect is more than 100 bounds, so a missing or misplaced mirror, a swapped order or side indices not reused for the
    mirrored view cannot pass."""
    cls_w = sds[version]["mlp_head.0.weight"]
    idx = np.array([0, 3, 5, 1, 4], np.int32) if side else None
    _load(eng, blobs, version, mode, chunk=2)
    try:
        eng.set_side_index(idx)
        e1 = eng.swin_embed_f32_nchw(x5)
        eng.set_side_index(idx)
        e2 = eng.swin_embed_f32_nchw(_flip(x5))
        eng.set_side_index(idx)
        got = eng.swin_descriptor_f32_nchw(x5, flip_tta=True)
        eng.set_side_index(idx)
        got_plain = eng.swin_descriptor_f32_nchw(x5, flip_tta=False)
        if side:
            unsided = eng.swin_embed_f32_nchw(x5)
            assert np.abs(unsided - e1).max() > 1e-3                       # the indices did reach the forward
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)
    assert got.shape == (5, 847) and np.isfinite(got).all()
    for what, g, (want, bound) in (("tta", got, ref.descriptor64(e1, e2, cls_w)), ("plain", got_plain, ref.descriptor64(e1, None, cls_w))):
        err = np.abs(g.astype(np.float64) - want)
        print("RATIO swin_descriptor entry %s mode %d side %d %s: worst err/bound %.4f, largest bound %.2e" %
              (version, mode, side, what, (err / bound).max(), bound.max()))
        assert (err <= bound).all(), "%s: worst err/bound %.3f" % (what, (err / bound).max())
        assert float(fx["tta_effect_" + version]) > 100 * bound.max()
        assert float(fx["side_effect_" + version]) > 100 * bound.max()
    assert np.abs(e1 - e2).max() > 0                                        # the views differ: the oracle's two inputs are two inputs


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_u8_entry_equals_f32_entry_on_host_preprocessed_crops(eng, blobs, version, mode):
    """reid_swin_descriptor_ragged_u8 against reid_swin_descriptor_f32_nchw on tests/swin_crops_ref.preprocess of the same crops: the
    same bits, with side indices, TTA on and off, in passes of 2, 2, 1."""
    _, crops, _ = cref.crop_set()
    crops = crops[3:8]
    idx = np.array([5, 0, 2, 2, 1], np.int32)
    ms = cref.OTHER_MEAN_STD
    pre = cref.preprocess(crops, SIZE, ms[:3], ms[3:])
    _load(eng, blobs, version, mode, chunk=2)
    try:
        for tta in (True, False):
            eng.set_side_index(idx)
            want = eng.swin_descriptor_f32_nchw(pre, flip_tta=tta)
            eng.set_side_index(idx)
            got = eng.swin_descriptor_ragged_u8(crops, size=SIZE, mean_std=ms, flip_tta=tta)
            np.testing.assert_array_equal(got, want, err_msg="tta %d" % tta)
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)


def test_side_index_count_mismatch_and_refusals(eng, blobs, x5):
    """4 side indices for 5 images: REID_ERR_ARG, and nothing stays pending - the next embed call runs without side information.  An
    index outside the table, a blob without classifier and n == 0 behave as include/reid_hip.h says."""
    _load(eng, blobs, "v1", 0, chunk=2)
    try:
        plain = eng.swin_embed_f32_nchw(x5[:2])
        for bad in (np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2, 3, VIEWS], np.int32)):
            eng.set_side_index(bad)
            with pytest.raises(_ffi.ReidHipError) as ei:
                eng.swin_descriptor_f32_nchw(x5)
            assert ei.value.status == -1 and "side ind" in str(ei.value)
            np.testing.assert_array_equal(eng.swin_embed_f32_nchw(x5[:2]), plain)      # 2 images: pending indices would raise or change it
        eng.set_side_index(np.array([1, 1], np.int32))
        assert eng.swin_descriptor_f32_nchw(x5[:0]).shape == (0, 847)                   # n == 0: OK ...
        np.testing.assert_array_equal(eng.swin_embed_f32_nchw(x5[:2]), plain)          # ... and nothing pending either
        eng.load_swin(*blobs["nocls"])
        out = np.empty((2, 96), np.float32)
        st = eng.lib.reid_swin_descriptor_f32_nchw(eng.h, x5.ctypes.data, 2, SIZE[0], SIZE[1], 1, out.ctypes.data)
        assert st == -3 and b"no classifier" in eng.lib.reid_last_error()
        st = eng.lib.reid_swin_descriptor_f32_nchw(eng.h, x5.ctypes.data, 2, 200, 224, 1, out.ctypes.data)
        assert st == -1
    finally:
        eng.set_side_index(None)
        eng.set_chunk(1024)


# ----------------------------------------------------------------------------- 5. against the reference
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_descriptors_match_the_reference(eng, fx, blobs, version, mode):
    """swin_eval.npz part (a): the reference's swin_t on cat(x, flip(x)) as the script calls it, compared with its float64 descriptors -
    4 images at 448 x 224 with view_index [0, 3, 5, 1], 3 images at 224 x 224 without, TTA on and off, chunk 2.
    Modes 0 and 2: atol = min(tta_effect, side_effect) / 16 from the fixture (the generator asserts that 100 x the reference's own
    fp32-vs-float64 noise is below it).  Mode 1: 1 - cos < 1e-4 per row, the project's bar for that mode."""
    atol = min(float(fx["tta_effect_" + version]), float(fx["side_effect_" + version])) / 16
    assert float(fx["ref_noise_" + version]) * 100 < atol
    _load(eng, blobs, version, mode, chunk=2)
    try:
        got = {}
        for tag, x, idx in (("a4", synth.images_f32(4, 5, h=448, w=224), fx["view_index"]), ("a3", synth.images_f32(3, 6), None)):
            for what, tta in (("tta", True), ("plain", False)):
                eng.set_side_index(idx)
                got[tag, what] = eng.swin_descriptor_f32_nchw(x, flip_tta=tta)
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)
    for (tag, what), g in got.items():
        want = fx["%s_%s_f64_%s" % (tag, what, version)]
        err = float(np.abs(g.astype(np.float64) - want).max())
        cos = (g * want).sum(1) / np.linalg.norm(g, axis=1) / np.linalg.norm(want, axis=1)
        print("swin_eval %s mode %d %s %s: max abs err %.3e (atol %.3e), 1 - cos %.3e" % (version, mode, tag, what, err, atol, (1 - cos).max()))
        if mode == 1:
            assert (1 - cos).max() < 1e-4, (tag, what)
        else:
            assert err <= atol, (tag, what, err, atol)


# ----------------------------------------------------------------------------- 6. the chain
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_chain_matches_the_reference_chain(eng, fx, blobs, version):
    """evaluate_reid(arch="swin", use_side=True) against swin_eval.npz part (c) - the script's chain through the reference's own swin_t,
    diminish_camera_bias, compute_jaccard_distance, DBSCAN, smooth_tracklets and evaluate_all on 48 gallery + 12 query images at
    448 x 224 - held to the bars of the ResNet chain test (tests/test_gpu_parity.py::test_e2e_harness_matches_reference_chain)."""
    from reid_amd import reid_inference
    seed, step = int(fx["chain_seed"]), int(fx["chain_row_step"])
    sizes = {k: int(fx["chain_" + k]) for k in ("n_ids", "n_cams", "n_gallery", "n_query")}
    prob = synth.e2e_problem(seed, **sizes)
    g_img = synth.identity_images_f32(prob["gl"], prob["gc"], seed + 1, h=448, w=224)
    q_img = synth.identity_images_f32(prob["ql"], prob["qc"], seed + 2, h=448, w=224)
    _load(eng, blobs, version, 0)
    taps = {}
    args = (g_img, prob["gl"], prob["gc"], prob["gs"], q_img, prob["ql"], prob["qc"], prob["qs"])
    cmc, mean_ap = reid_inference.evaluate_reid(*args, num_gallery_cams=sizes["n_cams"], eps=float(fx["chain_eps_" + version]), taps=taps,
                                                verbose=False, engine=eng, arch="swin", use_side=True)
    g = {k: fx["chain_%s_%s" % (k, version)] for k in ("desc", "debiased", "jaccard", "smoothed", "pseudo_labels", "cmc", "map")}
    for k in ("desc", "debiased", "jaccard", "smoothed"):
        print("swin_eval chain %s %s: max abs err %.3e" % (version, k, np.abs(taps[k][::step] - g[k]).max()))
    assert taps["desc"].shape == (sizes["n_gallery"] + sizes["n_query"], 847)
    np.testing.assert_allclose(taps["desc"][::step], g["desc"], atol=2e-5)
    np.testing.assert_allclose(taps["debiased"][::step], g["debiased"], atol=5e-5)
    np.testing.assert_allclose(taps["jaccard"][::step], g["jaccard"], atol=2e-4)
    assert float(fx["chain_eps_margin_" + version]) >= 5 * 2e-4        # eps sits in a gap of the reference's distances: same neighbourhoods
    assert (taps["pseudo_labels"] == g["pseudo_labels"]).all()
    np.testing.assert_allclose(taps["smoothed"][::step], g["smoothed"], atol=5e-5)
    np.testing.assert_array_equal(cmc, g["cmc"])
    assert abs(mean_ap - float(g["map"])) < 1e-6
    cmc2, map2 = reid_inference.evaluate_reid(*args, cluster_fn=lambda d: g["pseudo_labels"], verbose=False, engine=eng, arch="swin",
                                              use_side=True)
    np.testing.assert_array_equal(cmc2, cmc)
    assert map2 == mean_ap
