"""ResNet18-IBN-SE at any input size on the MI355X (pytest -m gpu tests/test_gpu_anysize.py).

Kernels: the three families of libreid_hip_anysize.so through the launchers the forward calls (reid_debug_any_norm / _se_tail / _gem)
against the float64 restatement of tests/anysize_ref.py with its derived per-element bounds (module docstring there); every output has
a guard pixel behind it that must still read as NaN, and what a launch must leave alone is given as NaN and must come back as NaN.

Forward: stage taps, embeddings, logits and descriptors of the three cases of tests/golden/anysize.npz (the reference's own class on the
CPU, tools/gen_golden_anysize.py).  The limits are the ones tests/test_gpu_parity.py applies to mode 0 at 256 x 128: a stage within 2e-5
of the oracle's largest magnitude (_seres18_fixture_check), embeddings and logits within 5e-5 of the fixture's largest magnitude and
1 - cosine below 1e-5 (same function), a descriptor within 2e-5 absolute (test_tta_descriptor_matches_oracle).  The fixture holds the
taps sampled (oracle/gen_golden._sample), so every stage is also compared in full against oracle/seres18.py, as that test does.

Generic path at 256 x 128: with the debug switch anysize_force the same limits against tests/golden/seres18_seed0.npz; without it the
reid_*_hw entries return the bits of the entries without a size, in every precision mode.

Equalities: passes of different sizes, host and device entries, uint8 images against PIL-resized floats - all bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import matching, seres18
from reid_amd import _ffi, synth, weights
from reid_amd.engine import stage_shapes
from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_ref as ref  # noqa: E402
import pil_resize_ref  # noqa: E402

pytestmark = [pytest.mark.gpu]

STAGE_LIMIT, EMB_LIMIT, COS_LIMIT, DESC_LIMIT = 2e-5, 5e-5, 1e-5, 2e-5      # tests/test_gpu_parity.py, mode 0 (module docstring)
NAMES_REF = ["bn0", "pooling0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["avgpooling"]
NAMES_ORACLE = ["stem", "pool0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["gem"]
HWS = (8, 30, 108, 238, 3752)
CS = (64, 512)
N = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.debug_switch("anysize_force", 0)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_precision(0)
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
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    return eng


def _embed_hw(eng, x, logits=True):
    """reid_embed_f32_nchw_hw itself, also at 256 x 128 (Engine.embed_f32_nchw hands that size to the entry without one)."""
    x = np.ascontiguousarray(x, np.float32)
    n, _, h, w = x.shape
    emb = np.empty((n, 512), np.float32)
    lg = np.empty((n, eng.num_class), np.float32) if logits else None
    _ffi.check(eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(x), n, h, w, _p(emb), _p(lg)))
    return (emb, lg) if logits else emb


def _descriptor_hw(eng, x, flip):
    x = np.ascontiguousarray(x, np.float32)
    n, _, h, w = x.shape
    out = np.empty((n, 512 + eng.num_class), np.float32)
    _ffi.check(eng.lib.reid_descriptor_f32_nchw_hw(eng.h, _p(x), n, h, w, int(flip), _p(out)))
    return out


def _case_input(fx, k):
    p = "c%d_" % k
    h, w, n, seed = (int(fx[p + key]) for key in ("h", "w", "n", "seed"))
    return p, h, w, n, seed, seres18.preprocess_u8(synth.smooth_crops_u8(n, seed, h, w))


def _sample_nhwc(flat, n, shape):
    """gen_golden._sample of a stage the engine hands back as flat NHWC."""
    ho, wo, c = shape
    t = flat.reshape(n, ho, wo, c).transpose(0, 3, 1, 2)
    return t[:, :: max(1, c // 8), :: max(1, ho // 8), :: max(1, wo // 4)]


# ---------------------------------------------------------------------------------------------- 1. kernels
def _kernel_data(hw, c, seed):
    rng = np.random.default_rng(seed * 100003 + hw * 7 + c)
    x = (rng.normal(0.3, 1.0, (N, hw, c)) * rng.uniform(0.5, 2.0, (1, 1, c))).astype(np.float32)
    return rng, x


def _held(got, want, bound, what):
    assert not np.isnan(got).any(), what + ": an output was left unwritten (or is NaN)"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), worst))
    assert (err <= bound).all(), "%s: err / bound %.3g" % (what, worst)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", HWS)
def test_norm_kernel(eng, hw, c):
    rng, x = _kernel_data(hw, c, 1)
    half = c // 2
    gamma, beta = rng.uniform(0.5, 1.5, half).astype(np.float32), rng.normal(0, 0.2, half).astype(np.float32)
    s, t = rng.uniform(0.5, 1.5, c - half).astype(np.float32), rng.normal(0, 0.2, c - half).astype(np.float32)
    want, bound = ref.instance_norm(x, gamma, beta, half, s, t)
    got = eng.debug_any_norm(x, half, gamma, beta, s, t)
    assert np.isnan(got[x.size:]).all(), "the guard pixel was written"
    _held(got[:x.size].reshape(x.shape), want, bound, "norm + BatchNorm half, hw %d c %d" % (hw, c))
    # BatchNorm half finished by the producer: those channels are not touched (given as NaN, they come back as NaN)
    x2 = x.copy()
    x2[:, :, half:] = np.nan
    got2 = eng.debug_any_norm(x2, half, gamma, beta)
    assert np.isnan(got2[x.size:]).all()
    got2 = got2[:x.size].reshape(x.shape)
    assert np.isnan(got2[:, :, half:]).all(), "the BatchNorm half was touched"
    assert np.array_equal(_bits(got2[:, :, :half]), _bits(got[:x.size].reshape(x.shape)[:, :, :half]))


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", HWS)
def test_se_tail_kernel(eng, hw, c):
    rng, y = _kernel_data(hw, c, 2)
    sc = rng.normal(0, 1, y.shape).astype(np.float32)
    mid = max(c // 16, 8)
    w1 = rng.normal(0, 1 / np.sqrt(c), (mid, c)).astype(np.float32)
    w2t = rng.normal(0, 1 / np.sqrt(mid), (mid, c)).astype(np.float32)
    want, gate, bound, gbound = ref.se_tail(y, sc, w1, w2t)
    out, g = eng.debug_any_se_tail(y, sc, w1, w2t)
    assert np.isnan(out[y.size:]).all() and np.isnan(g[N * c:]).all(), "a guard pixel was written"
    _held(g[:N * c].reshape(N, c), gate, gbound, "SE gate, hw %d c %d" % (hw, c))
    _held(out[:y.size].reshape(y.shape), want, bound, "SE tail, hw %d c %d" % (hw, c))


@pytest.mark.parametrize("p", [3.0, 2.6])
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", HWS)
def test_gem_kernel(eng, hw, c, p):
    rng, x = _kernel_data(hw, c, 3)
    x[0, 0, :] = 0.0
    scale, shift = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.2, c).astype(np.float32)
    g_want, e_want, gbound, ebound = ref.gem(x, p, scale, shift)
    g, e = eng.debug_any_gem(x, p, scale, shift)
    assert np.isnan(g[N * c:]).all() and np.isnan(e[N * c:]).all(), "a guard pixel was written"
    _held(g[:N * c].reshape(N, c), g_want, gbound, "GeM, hw %d c %d p %g" % (hw, c, p))
    _held(e[:N * c].reshape(N, c), e_want, ebound, "BNNeck, hw %d c %d p %g" % (hw, c, p))


# ---------------------------------------------------------------------------------------------- 2. forward
def _check_forward(eng, sd, x, emb_want, logits_want, sampled_taps, embed):
    """Taps, embeddings and logits of one pass under tests/test_gpu_parity.py's mode-0 limits; embed(x) -> (emb, logits)."""
    n, _, h, w = x.shape
    shapes = stage_shapes(h, w) + [(1, 1, 512)]
    eng.debug_keep(True)
    try:
        emb, logits = embed(x.numpy())
        taps = {}
        ref_emb, ref_logits = seres18.forward(sd, x, taps)
        for s, (name, rname) in enumerate(zip(NAMES_ORACLE, NAMES_REF)):
            t = taps[name]
            want = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1) if t.dim() == 4 else t.numpy().reshape(-1)
            got = eng.debug_stage(s, n, size=(h, w))
            err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
            print("stage %d (%s): rel max err %.3g against the oracle" % (s, name, err))
            assert err < STAGE_LIMIT, "stage %d (%s): rel max err %g" % (s, name, err)
            ft = sampled_taps[rname]
            mine = _sample_nhwc(got, n, shapes[s])
            assert mine.shape == ft.shape, (s, mine.shape, ft.shape)
            ferr = np.abs(mine - ft).max() / max(1e-6, np.abs(want).max())
            assert ferr < STAGE_LIMIT, "stage %d (%s): rel max err %g against the fixture" % (s, rname, ferr)
    finally:
        eng.debug_keep(False)
    for mine, want, what in ((emb, emb_want, "emb"), (emb, ref_emb.numpy(), "emb / oracle"), (logits, logits_want, "logits")):
        err = np.abs(mine - want).max() / np.abs(want).max()
        print("%s: rel max err %.3g" % (what, err))
        assert err < EMB_LIMIT, what
    cos = (emb * emb_want).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(emb_want, axis=1)
    assert (1 - cos).max() < COS_LIMIT
    return emb, logits


@pytest.mark.parametrize("k", [0, 1, 2])
def test_forward_matches_reference_fixture(eng_w0, sd0, fx, k):
    eng = eng_w0
    p, h, w, n, seed, x = _case_input(fx, k)
    taps = {name: fx[p + "tap_" + name] for name in NAMES_REF}
    emb, logits = _check_forward(eng, sd0, x, fx[p + "emb"], fx[p + "logits"], taps, lambda a: eng.embed_f32_nchw(a, logits=True))
    again = eng.embed_f32_nchw(x.numpy())                                  # without the stage buffers: the same bits
    assert np.array_equal(_bits(again), _bits(emb))
    for flip, key in ((True, "desc_tta"), (False, "desc_plain")):
        got = eng.descriptor_f32_nchw(x.numpy(), flip_tta=flip)
        err = np.abs(got - fx[p + key]).max()
        print("%s: max |err| %.3g" % (key, err))
        assert got.shape == (n, 512 + 751) and err <= DESC_LIMIT
    # the mirrored view is read with reversed columns, so a host-flipped batch swaps the two views' roles and nothing else: the sum of
    # the two descriptors commutes, the averaged descriptor has the same bits
    flipped = np.ascontiguousarray(x.numpy()[:, :, :, ::-1])
    assert np.array_equal(_bits(eng.descriptor_f32_nchw(flipped, flip_tta=True)), _bits(eng.descriptor_f32_nchw(x.numpy(), flip_tta=True)))
    assert not np.array_equal(_bits(eng.embed_f32_nchw(flipped)), _bits(emb))


def test_model_and_extractor_at_another_size(eng_w0, sd0, fx):
    """models.seres18_ibn(...)(x) on [N, 3, 96, 72] and Extractor(size=(W, H), precision="f32"): the engine's bits, its mode left alone."""
    from reid_amd.backbone import seres18_ibn
    from reid_amd.extractor import Extractor
    eng = eng_w0
    p, h, w, n, seed, x = _case_input(fx, 1)
    want = eng.embed_f32_nchw(x.numpy())
    model = seres18_ibn(num_classes=751, loss="triplet")
    model.load_state_dict(sd0)
    assert model.precision == "f16x3"
    eng.set_precision(2)
    try:
        got = np.asarray(model(x.numpy()))
        assert eng.precision == 2 and model.precision == "f16x3"           # the call ran in exact fp32, nothing was demoted
    finally:
        eng.set_precision(0)
    assert np.array_equal(_bits(got), _bits(want))
    crops = synth.ragged_crops_u8(4, seed=5)
    ext = Extractor(sd0, size=(72, 96), precision="f32")
    assert ext.size == (72, 96) and ext.precision == "f32"
    feats = ext(crops)
    ref_x = matching.preprocess(crops, size=(72, 96))
    ref_emb, _ = seres18.forward(sd0, torch.from_numpy(ref_x))
    assert np.abs(feats - ref_emb.numpy()).max() / np.abs(ref_emb.numpy()).max() < EMB_LIMIT
    assert np.array_equal(_bits(feats), _bits(eng.embed_ragged_u8(crops, size=(96, 72))))


# ---------------------------------------------------------------------------------------------- 3. the generic path at 256 x 128
def test_generic_path_at_256x128(eng_w0, sd0, golden_dir):
    eng = eng_w0
    g = np.load(os.path.join(golden_dir, "seres18_seed0.npz"))
    x = seres18.preprocess_u8(synth.crops_u8(int(g["n"]), int(g["seed"])))
    taps = {name: g["tap_" + name] for name in NAMES_REF}
    old = eng.embed_f32_nchw(x.numpy(), logits=True)
    eng.debug_switch("anysize_force", 1)
    try:
        emb, logits = _check_forward(eng, sd0, x, g["emb"], g["logits"], taps, lambda a: _embed_hw(eng, a))
        assert not np.array_equal(_bits(emb), _bits(old[0])), "the switch did not reach the generic forward"
        assert np.array_equal(_bits(eng.embed_f32_nchw(x.numpy())), _bits(old[0]))      # the entry without a size ignores the switch
    finally:
        eng.debug_switch("anysize_force", 0)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_entries_without_the_switch_return_the_old_bits(eng_w0, mode):
    eng = eng_w0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(5, 4)).numpy()
    crops = synth.ragged_crops_u8(4, seed=6)
    images = [pil_resize_ref.formula_image(h, w, i) for i, (h, w) in enumerate(((90, 200), (64, 32), (257, 129)))]
    eng.set_precision(mode)
    try:
        old_e, old_l = eng.embed_f32_nchw(x, logits=True)
        new_e, new_l = _embed_hw(eng, x)
        assert np.array_equal(_bits(new_e), _bits(old_e)) and np.array_equal(_bits(new_l), _bits(old_l))
        for flip in (True, False):
            assert np.array_equal(_bits(_descriptor_hw(eng, x, flip)), _bits(eng.descriptor_f32_nchw(x, flip_tta=flip)))
        assert np.array_equal(_bits(eng.embed_ragged_u8(crops, size=(256, 128))), _bits(eng.embed_ragged_u8(crops)))
        assert np.array_equal(_bits(eng.descriptor_images_u8(images, size=(256, 128))), _bits(eng.descriptor_images_u8(images)))
    finally:
        eng.set_precision(0)


# ---------------------------------------------------------------------------------------------- 4. equalities
def test_results_do_not_depend_on_the_pass(eng_w0):
    """(96, 72): the pass-size rule gives chunk * 4.74 images, never fewer than 4, so passes of 1, 2 and 5 images are calls of 1, 2 and 5
    images; chunk 1 and 2 give passes of 4 and 9.  Seven images one way or the other: equal bits, embeddings, logits and descriptors."""
    eng = eng_w0
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


def test_host_and_device_entries_agree(eng_w0):
    eng = eng_w0
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


def test_uint8_images_equal_pil_resized_floats(eng_w0):
    """reid_descriptor_images_u8_hw at (96, 72) from sources of 3 different sizes, bit for bit the float entry on the same images resized
    as PIL does on the host (tests/pil_resize_ref.py); pending camera indices serve both views, as at 256 x 128."""
    eng = eng_w0
    images = [pil_resize_ref.formula_image(h, w, i) for i, (h, w) in enumerate(((90, 200), (64, 32), (257, 129), (90, 200)))]
    x = pil_resize_ref.preprocess(images, 96, 72)
    for flip in (True, False):
        want = eng.descriptor_f32_nchw(x, flip_tta=flip)
        assert np.array_equal(_bits(eng.descriptor_images_u8(images, flip_tta=flip, size=(96, 72))), _bits(want))
    try:
        eng.set_chunk(1)                                                   # passes of 4: two passes for 7 images
        seven = images + images[:3]
        want = eng.descriptor_f32_nchw(pil_resize_ref.preprocess(seven, 96, 72))
        assert np.array_equal(_bits(eng.descriptor_images_u8(seven, size=(96, 72))), _bits(want))
    finally:
        eng.set_chunk(1024)
    cams = np.asarray([2, 0, 5, 1], np.int32)
    eng.set_side_index(np.concatenate([cams, cams]))
    want = eng.descriptor_f32_nchw(x)
    eng.set_side_index(cams)
    got = eng.descriptor_images_u8(images, size=(96, 72))
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(eng.descriptor_f32_nchw(x))), "the camera bias did not apply"


def test_evaluate_reid_at_the_veri_geometry(eng_w0):
    """evaluate_reid(arch="seres18_hw") on float images of (224, 268) runs the chain; its descriptors are the float entry's."""
    from reid_amd import reid_inference
    eng = eng_w0
    rng = np.random.default_rng(100)
    gl, gc, gs = rng.integers(0, 4, 12), np.arange(12) % 2, rng.integers(0, 3, 12)
    ql, qc, qs = rng.integers(1, 4, 4), np.arange(4) % 2, rng.integers(0, 3, 4)
    gx = synth.identity_images_f32(gl, gc, 101, h=224, w=268)
    qx = synth.identity_images_f32(ql, qc, 102, h=224, w=268)
    taps = {}
    cmc, m_ap = reid_inference.evaluate_reid(gx, gl, gc, gs, qx, ql, qc, qs, engine=eng, arch="seres18_hw", taps=taps, verbose=False, k1=6, k2=3,
                                             cluster_fn=lambda d: np.zeros(d.shape[0], np.int64))
    assert cmc.shape == (12,) and 0.0 <= m_ap <= 1.0
    assert np.array_equal(_bits(taps["desc"][:12]), _bits(eng.descriptor_f32_nchw(gx)))


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(eng, sd0):
    x = np.zeros((1, 3, 96, 72), np.float32)
    out = np.empty((1, 512), np.float32)

    def status(h, w, arr=x):
        return eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(arr), 1, h, w, _p(out), None)

    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    assert status(96, 72) == 0
    for h, w in ((31, 72), (96, 31), (513, 72), (96, 513)):
        assert status(h, w) == -1 and "[32, 512]" in eng.lib.reid_last_error().decode()           # REID_ERR_ARG
    eng.set_precision(2)
    try:
        assert status(96, 72) == -1
        msg = eng.lib.reid_last_error().decode()
        assert "seres18_ibn" in msg and "mode 2" in msg
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.descriptor_f32_nchw(x)
        assert ei.value.status == -1
        with pytest.raises(_ffi.ReidHipError):
            eng.descriptor_images_u8([np.zeros((9, 7, 3), np.uint8)], size=(96, 72))
        with pytest.raises(_ffi.ReidHipError):
            eng.embed_ragged_u8([np.zeros((9, 7, 3), np.uint8)], size=(96, 72))
    finally:
        eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
    try:
        assert status(96, 72) == -1
        msg = eng.lib.reid_last_error().decode()
        assert "cares18_ibn" in msg and "mode 0" in msg
        big = np.zeros((1, 3, 256, 128), np.float32)
        assert status(256, 128, big) == 0                                   # 256 x 128 runs every architecture
    finally:
        eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    assert eng.fault_bits() == 0
