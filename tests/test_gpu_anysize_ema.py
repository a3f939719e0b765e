"""EMARes18-IBN at any input size on the MI355X (pytest -m gpu tests/test_gpu_anysize_ema.py).

Kernels: the EMA tail of libreid_hip_anysize_ema.so through the launcher the forward calls (reid_debug_any_ema_tail) against the float64
oracle of tests/anysize_ema_ref.py under its derived per-element bound (module docstring there): the sigmoid vectors, mu, rstd and the two
softmaxes are checked under their own bounds before the output; the guards behind the output and behind the workspace must still read as
NaN.  The kernels take softmax(agp(x1)) = softmax(GroupNorm bias) (csrc/anysize_ema.h); the oracle computes it the long way.

Forward: the three cases of tests/golden/anysize_ema.npz (the reference's own EMARes18_IBN on the CPU, tools/gen_golden_anysize_ema.py)
with reid_ctx_set_hw_ema 1, in hw_precision 0 and 2, under the project's any-size limits: a block tap within 2e-5 of the tap's maximum,
1 - cos < 1e-5, embedding 2e-5, logits 5e-5 (relative to the fixture's largest magnitude); (256, 128) through the any-size trunk against
the emares18_ibn fixture of tests/golden/siblings.npz.

Equalities, bit for bit: an image alone and in a batch, a call repeated, the per-channel-constant family's exact statement, (256, 128)
with the setting on and off, passes of different sizes, host and device entries, the uint8 entries and the frame pipeline, the centre shift
and the plain mirror.  Refusals: the setting off (both messages), a bad value, cares18_ibn with only hw_ema, the precision rule, the old
kernel at a map it cannot hold, the library file absent."""
import ctypes as C
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
import anysize_ema_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_LIMIT, COS_LIMIT, EMB_LIMIT, LOGIT_LIMIT = 2e-5, 1e-5, 2e-5, 5e-5          # the project's any-size limits (tests/test_gpu_anysize_ca.py)
BLOCKS = [b[0] for b in synth.SERES18_BLOCKS]
IDS = ["%dx%dx%d" % c for c in ref.CASES]
OLD_LDS_LIMIT = 150 * 1024                                                      # launch_ema_tail, csrc/attention_f32.hip


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _old_fits(h, w, c):
    cg = c // 32
    return (3 * cg * h * w + 2 * cg * (h + w) + 6 * cg) * 4 <= OLD_LDS_LIMIT


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.debug_switch("anysize_force", 0)
    e.debug_switch("any_ema", 1)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_hw_ema(False)
    e.set_hw_siblings(False)
    e.set_hw_precision(None)
    e.set_precision(0)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anysize_ema.npz"))


@pytest.fixture(scope="module")
def sd_ema():
    return synth.emares18_state_dict(0)


@pytest.fixture()
def eng_ema(eng, sd_ema):
    """emares18_ibn weights bound, mode 0, the setting on, exact fp32 at other sizes."""
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(sd_ema)[:2])
    eng.set_hw_siblings(False)
    eng.set_hw_ema(True)
    eng.set_hw_precision(None)
    yield eng
    eng.set_hw_ema(False)
    eng.set_hw_precision(None)


# ---------------------------------------------------------------------------------------------- 1. the kernels
def _held(got, want, bound, what):
    assert not np.isnan(got).any(), what + ": an element was left unwritten (or is NaN)"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), worst))
    assert (err <= bound).all(), "%s: err / bound %.3g" % (what, worst)


@pytest.fixture(scope="module")
def oracle_cache():
    """(case, n, family) -> operands, oracle and bounds: computed once, shared, never written to."""
    cache = {}

    def get(case, n, family):
        key = (case, n, family)
        if key not in cache:
            y, sc = ref.operands(case, n, family)
            prm = ref.make_prm(case[2], ref.CASES.index(case))
            want, bound = ref.tail(y, sc, prm), ref.bounds(y, sc, prm)
            for a in (y, sc, prm) + tuple(want.values()) + tuple(bound.values()):
                a.setflags(write=False)
            cache[key] = (y, sc, prm, want, bound)
        return cache[key]
    return get


def _run_tail(eng, y, sc, prm):
    """-> dict with the keys of ref.tail(); the two guards are checked here."""
    n, h, w, c = y.shape
    out, sig, small = eng.debug_any_ema_tail(y, sc, prm)
    assert out[y.size:].size == c and np.isnan(out[y.size:]).all(), "the guard pixel behind out was written"
    assert small[n * 4 * c:].size == c and np.isnan(small[n * 4 * c:]).all(), "the guard behind the workspace was written"
    small = small[:n * 4 * c].reshape(n, 4, c)
    return {"out": out[:y.size].reshape(y.shape), "sig": sig, "mu": small[:, 0], "rstd": small[:, 1], "s1": small[:, 2], "s2": small[:, 3]}


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("case,n", [(case, n) for case in ref.CASES for n in ref.BATCHES[case]],
                         ids=["%s-n%d" % (i, n) for i, case in zip(IDS, ref.CASES) for n in ref.BATCHES[case]])
def test_tail_kernels_against_float64(eng, oracle_cache, case, n, family):
    y, sc, prm, want, bound = oracle_cache(case, n, family)
    got = _run_tail(eng, y, sc, prm)
    what = "%s n %d %s" % (case, n, family)
    for name in ("sig", "mu", "rstd", "s1", "s2", "out"):                   # the intermediates first, the output last
        _held(got[name], want[name], bound[name], name + " " + what)
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[4], ref.CASES[6]], ids=[IDS[2], IDS[4], IDS[6]])
def test_an_image_alone_and_in_a_batch_and_again(eng, case):
    """Image 1 of a batch of three and the same image alone: equal bits of the output and of every intermediate; a second call: equal
    bits.  (56, 67, 64) and (128, 2, 128) split an image's sums over several blocks."""
    y, sc = ref.operands(case, 3, "normal", seed=3)
    prm = ref.make_prm(case[2], 7)
    three = _run_tail(eng, y, sc, prm)
    one = _run_tail(eng, y[1:2], sc[1:2], prm)
    again = _run_tail(eng, y, sc, prm)
    for name in ref.NAMES:
        assert np.array_equal(_bits(three[name][1]), _bits(one[name][0])), name
        assert np.array_equal(_bits(three[name]), _bits(again[name])), name


@pytest.mark.parametrize("case", [ref.CASES[3], ref.CASES[4], ref.CASES[5]], ids=[IDS[3], IDS[4], IDS[5]])
def test_constant_channels_exact_statement(eng, case):
    """One value per (image, channel): every row mean and every column mean IS that value (an fp64 sum of at most 128 equal floats is
    exact), so the H + W rows of sig are equal bits; p = (y sig_h) sig_w is one float per channel, mu is that float bit for bit (16384
    equal floats add exactly too), and s1 is softmax(GroupNorm bias) whatever the data.  Then p - mu = 0 and x1 is the GroupNorm bias
    exactly, so the gate is the same at every pixel whose 3 x 3 window lies inside the map: there the output repeats bit for bit."""
    h, w, c = case
    cg = c // 32
    y, sc = ref.operands(case, 3, "const")
    sc = np.ascontiguousarray(np.broadcast_to(sc[:, :1, :1], sc.shape))     # a constant shortcut, so that equal gates give equal outputs
    prm = ref.make_prm(c, 5)
    got = _run_tail(eng, y, sc, prm)
    sig = got["sig"]
    assert np.array_equal(_bits(sig), _bits(np.broadcast_to(sig[:, :1], sig.shape)))
    p = (y[:, 0, 0] * sig[:, 0]) * sig[:, h]
    assert p.dtype == np.float32 and np.array_equal(_bits(got["mu"]), _bits(p))
    gb = ref.unpack_prm(prm, cg)[5].astype(np.float64)
    s1 = ref._softmax(gb)
    tol = ref._dsoftmax(s1, gb, np.zeros(cg), cg)                           # the evaluation's roundings alone: the input is exact
    assert (np.abs(got["s1"] - np.tile(s1, 32)) <= np.tile(tol, 32)).all()
    assert np.array_equal(_bits(got["s1"]), _bits(np.broadcast_to(got["s1"][:1], got["s1"].shape)))
    if h > 2 and w > 2:
        inner = got["out"][:, 1:h - 1, 1:w - 1]
        assert np.array_equal(_bits(inner), _bits(np.broadcast_to(inner[:, :1, :1], inner.shape)))


def test_shapes_outside_the_range_are_refused(eng):
    for shape in ((1, 1, 4, 64), (1, 4, 129, 64), (1, 4, 4, 96)):
        z = np.zeros(shape, np.float32)
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.debug_any_ema_tail(z, z, np.zeros(ref.prm_size(shape[3] // 32), np.float32))
        assert ei.value.status == -1, shape
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("case", [c for c in ref.CASES if _old_fits(*c)], ids=[i for i, c in zip(IDS, ref.CASES) if _old_fits(*c)])
def test_old_kernel_agrees_under_the_tail_bound(eng, oracle_cache, case):
    """launch_ema_tail of attention_f32.hip (what any_ema 0 puts into the trunk) against the new tail on the same operands, wherever the
    old kernel's slab fits LDS: at most the sum of both bounds apart.  The old kernel's bound is ref.bounds(old=True): the same derivation
    with that kernel's fp32 sums, unfused multiply-adds and measured agp(x1)."""
    y, sc, prm, want, bound = oracle_cache(case, 3, "normal")
    old_bound = ref.bounds(y, sc, prm, old=True)["out"]
    new = _run_tail(eng, y, sc, prm)["out"]
    old = eng.debug_sibling_tail(2, prm, y, sc)
    _held(old, want["out"], old_bound, "old kernel %s" % (case,))
    apart = float((np.abs(old.astype(np.float64) - new) / (bound["out"] + old_bound)).max())
    print("old against new %s: max |diff| / (new bound + old bound) %.3g" % (case, apart))
    assert apart <= 1.0


def test_old_kernel_refuses_the_map_it_cannot_hold(eng):
    """(128, 128, 64): launch_ema_tail is an ARG refusal with nothing launched, not a fault."""
    case = ref.CASES[-1]
    assert not _old_fits(*case)
    z = np.zeros((1,) + case, np.float32)
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.debug_sibling_tail(2, ref.make_prm(case[2], 0), z, z)
    assert ei.value.status == -1
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 2. the forward
def _case_input(fx, k):
    p = "c%d_" % k
    h, w, n, seed = (int(fx[p + key]) for key in ("h", "w", "n", "seed"))
    return p, h, w, n, seres18.preprocess_u8(synth.smooth_crops_u8(n, seed, h, w))


def _sample_nhwc(flat, n, shape):
    """gen_golden._sample of a stage the engine hands back as flat NHWC."""
    ho, wo, c = shape
    t = flat.reshape(n, ho, wo, c).transpose(0, 3, 1, 2)
    return t[:, :: max(1, c // 8), :: max(1, ho // 8), :: max(1, wo // 4)]


def _limits(eng, fx, p, h, w, n, x):
    """Block taps, cosine, embedding, logits of one fixture case."""
    shapes = stage_shapes(h, w)
    eng.debug_keep(True)
    try:
        emb, logits = eng.embed_f32_nchw(x, logits=True)
        for i, name in enumerate(BLOCKS):
            want = fx[p + "tap_" + name]
            got = _sample_nhwc(eng.debug_stage(2 + i, n, size=(h, w)), n, shapes[2 + i])
            assert got.shape == want.shape, (name, got.shape, want.shape)
            err = np.abs(got - want).max() / np.abs(want).max()
            print("%s: rel max err %.3g" % (name, err))
            assert err < TAP_LIMIT, "%s: rel max err %g" % (name, err)
    finally:
        eng.debug_keep(False)
    ew, lw = fx[p + "emb"], fx[p + "logits"]
    cos = (emb * ew).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ew, axis=1)
    e_err, l_err = np.abs(emb - ew).max() / np.abs(ew).max(), np.abs(logits - lw).max() / np.abs(lw).max()
    print("1 - cos %.3g, emb %.3g, logits %.3g" % ((1 - cos).max(), e_err, l_err))
    assert (1 - cos).max() < COS_LIMIT and e_err < EMB_LIMIT and l_err < LOGIT_LIMIT
    return emb, logits


@pytest.mark.parametrize("hw_precision", [0, 2])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_forward_matches_reference_fixture(eng_ema, fx, k, hw_precision):
    eng = eng_ema
    p, h, w, n, x = _case_input(fx, k)
    eng.set_hw_precision(hw_precision)
    emb, _ = _limits(eng, fx, p, h, w, n, x.numpy())
    assert np.array_equal(_bits(eng.embed_f32_nchw(x.numpy())), _bits(emb))            # without the stage buffers: the same bits
    assert eng.fault_bits() == 0


def test_256x128_is_not_affected_by_the_setting(eng_ema):
    eng = eng_ema
    x = seres18.preprocess_u8(synth.smooth_crops_u8(4, 4)).numpy()
    on = eng.embed_f32_nchw(x, logits=True)
    on_d = eng.descriptor_f32_nchw(x)
    eng.set_hw_ema(False)
    off = eng.embed_f32_nchw(x, logits=True)
    assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(_bits(on[1]), _bits(off[1]))
    assert np.array_equal(_bits(on_d), _bits(eng.descriptor_f32_nchw(x)))


def test_generic_path_at_256x128(eng_ema, golden_dir):
    """anysize_force with the setting on: the any-size forward on 256 x 128 crops against the 256 x 128 forward under the limits above, and
    against the emares18_ibn fixture of tests/golden/siblings.npz (the reference's own class on these crops)."""
    eng = eng_ema
    sib = np.load(os.path.join(golden_dir, "siblings.npz"))
    n = 3
    x = seres18.preprocess_u8(synth.smooth_crops_u8(n, 7)).numpy()                     # the crops of tests/test_gpu_parity.py::_sibling_check
    eng.debug_keep(True)
    try:
        old_e, old_l = eng.embed_f32_nchw(x, logits=True)
        old_taps = [eng.debug_stage(2 + i, n).copy() for i in range(8)]
        eng.debug_switch("anysize_force", 1)
        emb = np.empty((n, 512), np.float32)
        lg = np.empty((n, eng.num_class), np.float32)
        _ffi.check(eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(x), n, 256, 128, _p(emb), _p(lg)))
        for i, name in enumerate(BLOCKS):
            got = eng.debug_stage(2 + i, n, size=(256, 128))
            err = np.abs(got - old_taps[i]).max() / np.abs(old_taps[i]).max()
            assert err < TAP_LIMIT, "%s: rel max err %g" % (name, err)
            want = sib["ema_tap_" + name]
            err = np.abs(_sample_nhwc(got, n, stage_shapes(256, 128)[2 + i]) - want).max() / np.abs(want).max()
            assert err < TAP_LIMIT, "%s against the reference: rel max err %g" % (name, err)
    finally:
        eng.debug_switch("anysize_force", 0)
        eng.debug_keep(False)
    for want_e, want_l in ((old_e, old_l), (sib["ema_emb"], sib["ema_logits"])):
        cos = (emb * want_e).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(want_e, axis=1)
        assert (1 - cos).max() < COS_LIMIT
        assert np.abs(emb - want_e).max() / np.abs(want_e).max() < EMB_LIMIT
        assert np.abs(lg - want_l).max() / np.abs(want_l).max() < LOGIT_LIMIT
    assert not np.array_equal(_bits(emb), _bits(old_e)), "the switch did not reach the generic forward"


def test_the_switch_any_ema_reaches_the_trunk(eng_ema):
    """any_ema 0 runs the 256 x 128 forward's EMA kernel in the any-size trunk: block taps and embeddings agree with any_ema 1 under the
    forward's limits, and the switch comes back.  At (512, 512) the old kernel's layer-1 slab (128 x 128 x 2) does not fit: an ARG refusal in
    the middle of the trunk, no fault, and the next call runs."""
    eng = eng_ema
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 12, 96, 72)).numpy()
    assert eng.debug_switch("any_ema") == 1
    eng.debug_keep(True)
    try:
        new = eng.embed_f32_nchw(x)
        new_taps = [eng.debug_stage(2 + i, 3, size=(96, 72)).copy() for i in range(8)]
        eng.debug_switch("any_ema", 0)
        old = eng.embed_f32_nchw(x)
        old_taps = [eng.debug_stage(2 + i, 3, size=(96, 72)).copy() for i in range(8)]
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.embed_f32_nchw(np.zeros((1, 3, 512, 512), np.float32))
        assert ei.value.status == -1
    finally:
        eng.debug_switch("any_ema", 1)
        eng.debug_keep(False)
    for i, (a, b) in enumerate(zip(new_taps, old_taps)):
        err = np.abs(a - b).max() / np.abs(b).max()
        print("%s, new tail against old: rel max err %.3g" % (BLOCKS[i], err))
        assert err < TAP_LIMIT
    assert np.abs(new - old).max() / np.abs(old).max() < EMB_LIMIT
    assert np.array_equal(_bits(eng.embed_f32_nchw(x)), _bits(new))
    assert eng.fault_bits() == 0


def test_results_do_not_depend_on_the_pass(eng_ema):
    """(224, 268): a pass is chunk * 32768 / 60032 images, so chunk 10, 6 and 2 give passes of 5, 3 and 1 - five images in 1, 2 and 5
    passes; and calls of 1 and 2 images.  Equal bits, embeddings and logits."""
    from reid_amd.engine import any_pass_size
    eng = eng_ema
    assert [any_pass_size(c, 224, 268) for c in (10, 6, 2)] == [5, 3, 1]
    x = seres18.preprocess_u8(synth.smooth_crops_u8(5, 21, 224, 268)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    try:
        for chunk in (10, 6, 2):
            eng.set_chunk(chunk)
            e, l = eng.embed_f32_nchw(x, logits=True)
            assert np.array_equal(_bits(e), _bits(want_e)) and np.array_equal(_bits(l), _bits(want_l)), chunk
    finally:
        eng.set_chunk(1024)
    for m in (1, 2):
        parts = [eng.embed_f32_nchw(x[i:i + m], logits=True) for i in range(0, 5, m)]
        assert np.array_equal(_bits(np.concatenate([q[0] for q in parts])), _bits(want_e)), m
        assert np.array_equal(_bits(np.concatenate([q[1] for q in parts])), _bits(want_l)), m


def test_model_and_extractor_at_another_size(eng_ema, sd_ema, fx):
    """emares18_ibn(hw_ema=True)(x) on [N, 3, 96, 72] in exact fp32 and fp32-class, Extractor(size=(W, H), hw_ema=True): the engine's
    bits; the engine's settings come back."""
    from reid_amd.backbone import emares18_ibn
    from reid_amd.extractor import Extractor
    eng = eng_ema
    p, h, w, n, x = _case_input(fx, 1)
    want = eng.embed_f32_nchw(x.numpy())
    eng.set_hw_precision(2)
    want_x3 = eng.embed_f32_nchw(x.numpy())
    eng.set_hw_precision(None)
    eng.set_hw_ema(False)
    for hw_precision, ref_bits in ((None, want), ("f16x3", want_x3)):
        model = emares18_ibn(num_classes=751, loss="triplet", hw_ema=True, hw_precision=hw_precision)
        model.load_state_dict(sd_ema)
        got = np.asarray(model(x.numpy()))
        assert np.array_equal(_bits(got), _bits(ref_bits)), hw_precision
        assert not eng.hw_ema and eng.hw_precision == -1
    assert not np.array_equal(_bits(want), _bits(want_x3))
    crops = synth.ragged_crops_u8(4, seed=5)
    ext = Extractor(sd_ema, size=(72, 96), precision="f32", hw_ema=True)
    feats = ext(crops)
    assert not eng.hw_ema
    eng.set_hw_ema(True)
    eng.set_precision(0)
    assert np.array_equal(_bits(feats), _bits(eng.embed_ragged_u8(crops, size=(96, 72))))


def test_host_and_device_entries_agree(eng_ema):
    eng = eng_ema
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


def test_uint8_entries_and_the_frame_pipeline_give_equal_bits(eng_ema, sd_ema):
    """embed_ragged_u8(size=), reid_embed_frame_u8_hw, frame_submit_hw + fetch and CameraStream(arch="emares18_hw", hw_ema=True,
    size=(128, 64)) on the same windows."""
    from reid_amd.tracking import CameraStream
    eng = eng_ema
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    boxes = np.asarray([[10, 20, 60, 140], [100, 30, 170, 200], [200, 50, 260, 130], [5, 5, 40, 90]], np.int32)
    crops = [np.ascontiguousarray(frame[y0:y1, x0:x1]) for x0, y0, x1, y1 in boxes]
    want = eng.embed_ragged_u8(crops, size=(128, 64))
    got = eng.embed_frame_u8(frame, boxes, size=(128, 64))
    assert np.array_equal(_bits(got), _bits(want))
    eng.frame_submit_hw(1, crops, (128, 64))
    eng.frame_cost(1, want_emb=True)
    assert np.array_equal(_bits(eng.frame_fetch(1)[0]), _bits(want))
    eng.set_hw_ema(False)                                                     # the stream class switches it on itself
    blob, manifest = weights.pack_seres18(sd_ema)[:2]
    cam = CameraStream(blob, manifest, max_tracks=16, own_context=False, match_stream=False, arch="emares18_hw", size=(128, 64), hw_ema=True)
    try:
        assert cam.eng is eng and eng.hw_ema
        cam.submit(crops)
        feats, cost, iou = cam.step([], np.zeros((0, 4)), np.zeros((len(crops), 4)))
        assert np.array_equal(_bits(feats), _bits(want))
    finally:
        cam.close(destroy=True)


def test_centre_shift_gives_the_bits_of_flip_tta(eng_ema):
    eng = eng_ema
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 31, 96, 72)).numpy()
    want = eng.descriptor_f32_nchw(x, flip_tta=True)
    got = eng.descriptor_f32_nchw_shift(x, np.full((3, 2), 10, np.int32), pad=10, fill=(-1.0, -1.0, -1.0))
    assert np.array_equal(_bits(got), _bits(want))


def test_evaluate_reid_runs_the_chain(eng_ema):
    from reid_amd import reid_inference
    eng = eng_ema
    eng.set_hw_ema(False)                                                     # the keyword sets it for the call and restores it
    rng = np.random.default_rng(100)
    gl, gc, gs = rng.integers(0, 4, 12), np.arange(12) % 2, rng.integers(0, 3, 12)
    ql, qc, qs = rng.integers(1, 4, 4), np.arange(4) % 2, rng.integers(0, 3, 4)
    gx = synth.identity_images_f32(gl, gc, 101, h=96, w=72)
    qx = synth.identity_images_f32(ql, qc, 102, h=96, w=72)
    taps = {}
    cmc, m_ap = reid_inference.evaluate_reid(gx, gl, gc, gs, qx, ql, qc, qs, engine=eng, arch="emares18_hw", hw_ema=True, taps=taps, verbose=False,
                                             k1=6, k2=3, cluster_fn=lambda d: np.zeros(d.shape[0], np.int64))
    assert cmc.shape == (12,) and np.isfinite(cmc).all() and (np.diff(cmc) >= 0).all() and 0.0 <= cmc[0] <= cmc[-1] <= 1.0 and 0.0 <= m_ap <= 1.0
    assert not eng.hw_ema
    eng.set_hw_ema(True)
    assert np.array_equal(_bits(taps["desc"][:12]), _bits(eng.descriptor_f32_nchw(gx)))


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals(eng, sd_ema):
    x = np.zeros((1, 3, 96, 72), np.float32)
    out = np.empty((1, 512), np.float32)

    def status():
        return eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(x), 1, 96, 72, _p(out), None)

    eng.set_precision(0)
    eng.set_hw_precision(None)
    eng.set_hw_siblings(False)
    eng.set_hw_ema(False)
    eng.load_seres18(*weights.pack_seres18(sd_ema)[:2])
    try:
        assert status() == -1                                               # the setting off: today's two messages, verbatim
        assert eng.lib.reid_last_error().decode() == (
            "reid_embed_f32_nchw_hw: input size 96 x 72 runs seres18_ibn in precision mode 0 (exact fp32) only; loaded architecture "
            "emares18_ibn, precision mode 0 (256 x 128 runs every architecture and mode)")
        eng.set_hw_siblings(True)
        assert status() == -1
        assert eng.lib.reid_last_error().decode() == (
            "reid_embed_f32_nchw_hw: input size 96 x 72: loaded architecture emares18_ibn has no any-size tail; with "
            "reid_ctx_set_hw_siblings 1 only cares18_ibn runs at sizes other than 256 x 128 beside seres18_ibn")
        assert eng.lib.reid_ctx_set_hw_ema(eng.h, 2) == -1 and eng.lib.reid_ctx_set_hw_ema(eng.h, -1) == -1
        assert status() == -1                                               # a refused value changed nothing
        eng.set_hw_ema(True)
        assert status() == 0                                                # whatever hw_siblings is
        eng.set_hw_siblings(False)
        assert status() == 0
        eng.set_precision(2)                                                # the precision rule of seres18_ibn: -1 needs mode 0
        assert status() == -1 and "mode 2" in eng.lib.reid_last_error().decode()
        eng.set_hw_precision(0)
        assert status() == 0
        eng.set_hw_precision(None)
        eng.set_precision(0)
        big = np.zeros((1, 3, 256, 128), np.float32)
        assert eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(big), 1, 256, 128, _p(out), None) == 0
        eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
        assert status() == -1                                               # cares18_ibn with only hw_ema: it still needs hw_siblings
        assert "cares18_ibn" in eng.lib.reid_last_error().decode()
        eng.set_hw_siblings(True)
        assert status() == 0
    finally:
        eng.set_precision(0)
        eng.set_hw_precision(None)
        eng.set_hw_siblings(False)
        eng.set_hw_ema(False)
    assert eng.fault_bits() == 0


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_seres18(*weights.pack_seres18(synth.emares18_state_dict(0))[:2])
eng.set_hw_ema(True)
x = np.zeros((1, 3, 96, 72), np.float32)
try:
    eng.embed_f32_nchw(x)
    print("RAN")
except _ffi.ReidHipError as e:
    print("STATUS", e.status, "NAMED", "libreid_hip_anysize_ema.so" in str(e))
try:
    eng.frame_submit_hw(0, [np.zeros((40, 20, 3), np.uint8)], (128, 64))
    print("RAN")
except _ffi.ReidHipError as e:
    print("SUBMIT", e.status, "NAMED", "libreid_hip_anysize_ema.so" in str(e))
big = eng.embed_f32_nchw(np.zeros((1, 3, 256, 128), np.float32))
print("BIG", big.shape, bool(np.isfinite(big).all()))
eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
eng.set_hw_siblings(True)
print("CA", eng.embed_f32_nchw(x).shape)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
print("SE", eng.embed_f32_nchw(x).shape)
print("FAULT", eng.fault_bits())
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_anysize_ema.so, loaded through REID_HIP_LIB in a fresh child process: an emares18_ibn call
    at another size is REID_ERR_STATE naming the file, the frame submit too (nothing queued), and every other call runs."""
    lib = "libreid_hip_anysize_ema.so"
    shutil.copytree(os.path.join(ROOT, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(ROOT, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "STATUS -3 NAMED True" in lines and "SUBMIT -3 NAMED True" in lines and "RAN" not in lines, r.stdout
    assert "BIG (1, 512) True" in lines and "CA (1, 512)" in lines and "SE (1, 512)" in lines and "FAULT 0" in lines, r.stdout
