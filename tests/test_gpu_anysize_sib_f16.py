"""CARes18-IBN and EMARes18-IBN at any input size in fp16 storage on the MI355X (pytest -m gpu tests/test_gpu_anysize_sib_f16.py).

Kernels: the TripletAttention and EMA tails of libreid_hip_anysize_sib_f16.so through the launchers the forward calls
(reid_debug_any_ca_tail_f16, reid_debug_any_ema_tail_f16) against the float64 oracles of tests/anysize_ca_ref.py / tests/anysize_ema_ref.py
on the f16-rounded operands (tests/anysize_sib_f16_ref.py): the returned fp32 statistics under b32, the f16 output under
store_bound(v, b32) = b32 + 2^-11 (|v| + b32) + 2^-25; the guards behind the output and behind the workspace still NaN, no output element
NaN, fault word 0; an image alone and in a batch, and a call repeated: equal bits; shapes outside the range refused with out untouched.

Forward: reid_ctx_set_hw_sib_f16 1 on the three cases of tests/golden/anysize_ca.npz and anysize_ema.npz under the mode-1 limits
(anysize_f16_ref.COS_LIMIT / EMB_LIMIT / STAGE_LIMIT); bit-for-bit equalities between pass sizes, host and device entries, the uint8
entries, the frame pipeline, CameraStream, the centre shift and (256, 128); the setting's rules; the library file absent.

Measured on an MI355X (profiles/anysize_sib_f16_gpu_tests.log) - the limits are the derived ones, not these:
worst err / bound per kernel - TripletAttention: maps 0.99, gates 0.16, out 0.995; EMA: sig 0.56, mu 0.23, rstd 0.79, s1 0.12, s2 0.11, out 0.999
(the half-ulp of an f16 value at the bottom of its binade IS 2^-11 |v|, so a correct store gets this close; the statistics' bounds are b32).
Forward, 1 - cos / embedding / logits / worst block tap (fractions of the largest magnitude):
  cares18_ibn   (64, 32) 1.8e-7 / 8.3e-4 / 5.1e-4 / 1.3e-3;  (96, 72) 6.0e-8 / 3.9e-4 / 3.5e-4 / 1.5e-3;  (224, 268) 1.2e-7 / 1.9e-4 / 2.6e-4 / 1.1e-3
  emares18_ibn  (64, 32) 1.8e-7 / 4.5e-4 / 3.9e-4 / 1.5e-3;  (96, 72) 0 / 4.2e-4 / 3.1e-4 / 2.6e-3;  (224, 268) 0 / 4.1e-4 / 2.8e-4 / 2.2e-3
"""
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
import anysize_sib_f16_ref as r  # noqa: E402

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [b[0] for b in synth.SERES18_BLOCKS]
SIZE = (96, 72)
MAKE_SD = {"cares18_ibn": synth.cares18_state_dict, "emares18_ibn": synth.emares18_state_dict}
HW_ARCH = {"cares18_ibn": "cares18_hw", "emares18_ibn": "emares18_hw"}
SIBS = tuple(MAKE_SD)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _defaults(e):
    e.set_hw_sib_f16(False)           # without the feature the module fails here, at its first use of reid_ctx_set_hw_sib_f16
    e.clear_fault()
    e.debug_switch("anysize_force", 0)
    e.debug_keep(False)
    e.set_side_index(None)
    e.set_precision(0)
    e.set_hw_precision(-1)
    e.set_hw_siblings(False)
    e.set_hw_ema(False)
    e.set_hw_f16(False)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def sds():
    return {a: MAKE_SD[a](0) for a in SIBS}


@pytest.fixture(scope="module")
def blobs(sds):
    return {a: weights.pack_seres18(sds[a])[:2] for a in SIBS}


@pytest.fixture(scope="module")
def blob_se():
    return weights.pack_seres18(synth.seres18_state_dict(0))[:2]


@pytest.fixture(scope="module")
def eng(blob_se):
    from reid_amd.engine import get_engine
    e = get_engine(0)
    _defaults(e)
    yield e
    _defaults(e)
    e.load_seres18(*blob_se)


@pytest.fixture()
def eng0(eng):
    _defaults(eng)
    yield eng
    assert eng.fault_bits() == 0
    _defaults(eng)


@pytest.fixture(scope="module")
def fxs(golden_dir):
    return {a: np.load(os.path.join(golden_dir, f)) for a, f in r.ARCHS.items()}


def _load(eng, blobs, arch, on=True):
    eng.load_seres18(*blobs[arch])
    eng.set_hw_sib_f16(on)
    return eng


# ---------------------------------------------------------------------------------------------- 1. the kernels
def _held(got, want, bound, what):
    assert not np.isnan(got).any(), what + ": an element was left unwritten (or is NaN)"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), worst))
    assert (err <= bound).all(), "%s: err / bound %.3g" % (what, worst)


@pytest.fixture(scope="module")
def case_cache():
    """(kind, case, n, family) -> operands, oracle and bounds: computed once, shared, never written to."""
    cache = {}

    def get(kind, case, n, family):
        key = (kind, case, n, family)
        if key not in cache:
            d = r.ca_case(case, n, family) if kind == "ca" else r.ema_case(case, n, family)
            for a in d.values():
                for b in (a.values() if isinstance(a, dict) else (a,)):
                    b.setflags(write=False)
            cache[key] = d
        return cache[key]
    return get


def _run_ca(eng, y, sc, prm):
    n, h, w, c = y.shape
    per = h * w + c * w + h * c
    out, maps, gates = eng.debug_any_ca_tail_f16(y, sc, prm)
    assert out[y.size:].size == c and np.isnan(out[y.size:]).all(), "the guard pixel behind out was written"
    assert gates[n * per:].size == c and np.isnan(gates[n * per:]).all(), "the guard behind the workspace was written"
    return {"out": out[:y.size].reshape(y.shape), "maps": maps, "gates": gates[:n * per].reshape(n, per)}


def _run_ema(eng, y, sc, prm):
    n, h, w, c = y.shape
    out, sig, small = eng.debug_any_ema_tail_f16(y, sc, prm)
    assert out[y.size:].size == c and np.isnan(out[y.size:]).all(), "the guard pixel behind out was written"
    assert small[n * 4 * c:].size == c and np.isnan(small[n * 4 * c:]).all(), "the guard behind the workspace was written"
    small = small[:n * 4 * c].reshape(n, 4, c)
    return {"out": out[:y.size].reshape(y.shape), "sig": sig, "mu": small[:, 0], "rstd": small[:, 1], "s1": small[:, 2], "s2": small[:, 3]}


@pytest.mark.parametrize("family", r.CA_FAMILIES)
@pytest.mark.parametrize("case,n", [(case, n) for case in r.CA_CASES for n in r.batches(case)],
                         ids=["%dx%dx%d-n%d" % (case + (n,)) for case in r.CA_CASES for n in r.batches(case)])
def test_ca_tail_against_float64(eng0, case_cache, case, n, family):
    d = case_cache("ca", case, n, family)
    got = _run_ca(eng0, d["y"], d["sc"], d["prm"])
    what = "CA %s n %d %s" % (case, n, family)
    _held(got["maps"], d["maps"], d["b_maps"], "maps " + what)              # the statistics first, under b32 unchanged
    _held(got["gates"], d["gates"], d["b_gates"], "gates " + what)
    _held(got["out"], d["out"], d["b_out"], "out " + what)
    assert eng0.fault_bits() == 0


@pytest.mark.parametrize("family", r.EMA_FAMILIES)
@pytest.mark.parametrize("case,n", [(case, n) for case in r.EMA_CASES for n in r.batches(case)],
                         ids=["%dx%dx%d-n%d" % (case + (n,)) for case in r.EMA_CASES for n in r.batches(case)])
def test_ema_tail_against_float64(eng0, case_cache, case, n, family):
    d = case_cache("ema", case, n, family)
    got = _run_ema(eng0, d["y"], d["sc"], d["prm"])
    what = "EMA %s n %d %s" % (case, n, family)
    for name in ("sig", "mu", "rstd", "s1", "s2"):
        _held(got[name], d["want"][name], d["b32"][name], name + " " + what)
    _held(got["out"], d["want"]["out"], d["b_out"], "out " + what)
    assert eng0.fault_bits() == 0


@pytest.mark.parametrize("kind,case", [("ca", r.CA_CASES[3]), ("ca", r.CA_CASES[4]), ("ema", r.EMA_CASES[2]), ("ema", r.EMA_CASES[4]),
                                       ("ema", r.EMA_CASES[6]), ("ema", r.EMA_CASES[0])],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_an_image_alone_and_in_a_batch_and_again(eng0, kind, case):
    """Image 0 of the n = 3 call and the same image alone: equal bits of the output and of every statistic; three calls: equal bits."""
    ops, run = (r.ca_operands, _run_ca) if kind == "ca" else (r.ema_operands, _run_ema)
    y, sc, prm = ops(case, 3, r.CA_FAMILIES[0] if kind == "ca" else r.EMA_FAMILIES[0], seed=3)
    three = run(eng0, y, sc, prm)
    one = run(eng0, y[:1], sc[:1], prm)
    for name in three:
        same = _bits16 if name == "out" else _bits
        assert np.array_equal(same(three[name][0]), same(one[name][0])), name
    for _ in range(2):
        again = run(eng0, y, sc, prm)
        for name in three:
            same = _bits16 if name == "out" else _bits
            assert np.array_equal(same(three[name]), same(again[name])), name


def test_shapes_outside_the_range_are_refused(eng0):
    for shape in ((1, 1, 4, 64), (1, 4, 129, 64), (1, 4, 4, 96)):
        z = np.zeros(shape, np.float16)
        for run, prm in ((eng0.debug_any_ca_tail_f16, np.zeros(300, np.float32)),
                         (eng0.debug_any_ema_tail_f16, np.zeros((shape[3] // 32) ** 2 * 10 + 4 * (shape[3] // 32), np.float32))):
            out = np.full(z.size + shape[3], 7.0, np.float16)
            with pytest.raises(_ffi.ReidHipError) as ei:
                run(z, z, prm, out=out)
            assert ei.value.status == -1, shape
            assert (out == 7.0).all(), "a refused call wrote its output"
    assert eng0.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 2. the forward
def _case_input(fx, k):
    p = "c%d_" % k
    h, w, n, seed = (int(fx[p + key]) for key in ("h", "w", "n", "seed"))
    return p, h, w, n, seres18.preprocess_u8(synth.smooth_crops_u8(n, seed, h, w))


def _sample_nhwc(flat, n, shape):
    ho, wo, c = shape
    t = flat.reshape(n, ho, wo, c).transpose(0, 3, 1, 2)
    return t[:, :: max(1, c // 8), :: max(1, ho // 8), :: max(1, wo // 4)]


def _cos_err(a, b):
    return float((1.0 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)).max())


@pytest.mark.parametrize("k", r.FORWARD_CASES)
@pytest.mark.parametrize("arch", SIBS)
def test_forward_matches_reference_fixture(eng0, blobs, fxs, arch, k):
    eng, fx = eng0, fxs[arch]
    p, h, w, n, x = _case_input(fx, k)
    xn = x.numpy()
    eng.load_seres18(*blobs[arch])
    eng.set_hw_siblings(True)
    eng.set_hw_ema(True)
    eng.set_hw_precision(0)
    exact = eng.embed_f32_nchw(xn)
    eng.set_hw_precision(2)
    class3 = eng.embed_f32_nchw(xn)
    eng.set_hw_sib_f16(True)                                  # hw_precision stays 2: the new setting wins
    shapes = stage_shapes(h, w)
    eng.debug_keep(True)
    try:
        emb, logits = eng.embed_f32_nchw(xn, logits=True)
        worst = 0.0
        for i, name in enumerate(BLOCKS):
            want = fx[p + "tap_" + name]
            flat = eng.debug_stage(2 + i, n, size=(h, w))
            assert np.array_equal(flat, flat.astype(np.float16).astype(np.float32)), "%s: the tap does not survive a float16 round trip" % name
            got = _sample_nhwc(flat, n, shapes[2 + i])
            assert got.shape == want.shape, (name, got.shape, want.shape)
            err = np.abs(got - want).max() / np.abs(want).max()
            print("%s %s: rel max err %.3g" % (arch, name, err))
            assert err < r.STAGE_LIMIT, "%s: rel max err %g" % (name, err)
            worst = max(worst, err)
    finally:
        eng.debug_keep(False)
    ce = _cos_err(emb, fx[p + "emb"])
    ee = np.abs(emb - fx[p + "emb"]).max() / np.abs(fx[p + "emb"]).max()
    le = np.abs(logits - fx[p + "logits"]).max() / np.abs(fx[p + "logits"]).max()
    print("%s (%d, %d): 1 - cos %.3g, emb %.3g, logits %.3g, worst tap %.3g" % (arch, h, w, ce, ee, le, worst))
    assert ce < r.COS_LIMIT and ee < r.EMB_LIMIT and le < r.EMB_LIMIT
    assert np.array_equal(_bits(eng.embed_f32_nchw(xn)), _bits(emb))           # without the stage buffers: the same bits
    assert not np.array_equal(_bits(emb), _bits(exact)), "hw_sib_f16 returned the bits of hw_precision 0"
    assert not np.array_equal(_bits(emb), _bits(class3)), "hw_sib_f16 returned the bits of hw_precision 2"


# ---------------------------------------------------------------------------------------------- 3. equalities, bit for bit
@pytest.mark.parametrize("arch", SIBS)
def test_results_do_not_depend_on_the_pass(eng0, blobs, arch):
    """(224, 268): a pass is chunk * 32768 / 60032 images, so chunk 6 and 2 give passes of 3 and 1; and calls of one image."""
    from reid_amd.engine import any_pass_size
    eng = _load(eng0, blobs, arch)
    assert [any_pass_size(c, 224, 268) for c in (6, 2)] == [3, 1]
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 21, 224, 268)).numpy()
    want_e, want_l = eng.embed_f32_nchw(x, logits=True)
    try:
        for chunk in (6, 2):
            eng.set_chunk(chunk)
            e, l = eng.embed_f32_nchw(x, logits=True)
            assert np.array_equal(_bits(e), _bits(want_e)) and np.array_equal(_bits(l), _bits(want_l)), chunk
    finally:
        eng.set_chunk(1024)
    parts = [eng.embed_f32_nchw(x[i:i + 1], logits=True) for i in range(3)]
    assert np.array_equal(_bits(np.concatenate([q[0] for q in parts])), _bits(want_e))
    assert np.array_equal(_bits(np.concatenate([q[1] for q in parts])), _bits(want_l))


@pytest.mark.parametrize("arch", SIBS)
def test_host_and_device_entries_and_the_shift_agree(eng0, blobs, arch):
    eng = _load(eng0, blobs, arch)
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
    tta = eng.descriptor_f32_nchw(x[:3], flip_tta=True)
    got = eng.descriptor_f32_nchw_shift(x[:3], np.full((3, 2), 10, np.int32), pad=10, fill=(-1.0, -1.0, -1.0))
    assert np.array_equal(_bits(got), _bits(tta))
    eng.set_hw_sib_f16(False)
    eng.set_hw_siblings(True)
    eng.set_hw_ema(True)
    assert not np.array_equal(_bits(eng.descriptor_f32_nchw(x)), _bits(want_d))


@pytest.mark.parametrize("arch", SIBS)
def test_uint8_entries_frame_pipeline_and_stream_give_equal_bits(eng0, blobs, arch):
    """embed_ragged_u8(size=) against embed_f32_nchw on the same crops preprocessed in fp32 (crops already at the size: the resize is the
    identity), reid_embed_frame_u8_hw, frame_submit_hw + frame_cost(want_emb=True), and CameraStream(arch=, hw_sib_f16=True)."""
    from reid_amd.tracking import CameraStream
    eng = _load(eng0, blobs, arch)
    at_size = synth.smooth_crops_u8(3, 9, 128, 64)
    want_same = eng.embed_f32_nchw(seres18.preprocess_u8(at_size).numpy())
    assert np.array_equal(_bits(eng.embed_ragged_u8(list(at_size), size=(128, 64))), _bits(want_same))
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    boxes = np.asarray([[10, 20, 60, 140], [100, 30, 170, 200], [200, 50, 260, 130], [5, 5, 40, 90]], np.int32)
    crops = [np.ascontiguousarray(frame[y0:y1, x0:x1]) for x0, y0, x1, y1 in boxes]
    want = eng.embed_ragged_u8(crops, size=(128, 64))
    assert np.array_equal(_bits(eng.embed_frame_u8(frame, boxes, size=(128, 64))), _bits(want))
    eng.frame_submit_hw(1, crops, (128, 64))
    eng.frame_cost(1, want_emb=True)
    assert np.array_equal(_bits(eng.frame_fetch(1)[0]), _bits(want))
    eng.set_hw_sib_f16(False)                                                 # the stream class switches it on itself
    eng.set_hw_siblings(True)
    eng.set_hw_ema(True)
    eng.set_hw_precision(0)
    assert not np.array_equal(_bits(eng.embed_ragged_u8(crops, size=(128, 64))), _bits(want)), "the fp32 forward gave the same bits"
    eng.set_hw_siblings(False)
    eng.set_hw_ema(False)
    eng.set_hw_precision(-1)
    cam = CameraStream(*blobs[arch], max_tracks=16, own_context=False, match_stream=False, arch=HW_ARCH[arch], size=(128, 64),
                       hw_sib_f16=True, **({"hw_ema": True} if arch == "emares18_ibn" else {}))
    try:
        assert cam.eng is eng and eng.hw_sib_f16 is True
        cam.submit(crops)
        feats, cost, iou = cam.step([], np.zeros((0, 4)), np.zeros((len(crops), 4)))
        assert np.array_equal(_bits(feats), _bits(want))
    finally:
        cam.close(destroy=True)


@pytest.mark.parametrize("arch", SIBS)
def test_256x128_is_not_affected(eng0, blobs, arch):
    eng = eng0
    eng.load_seres18(*blobs[arch])
    big = seres18.preprocess_u8(synth.smooth_crops_u8(3, 24)).numpy()
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        eng.set_hw_sib_f16(False)
        before = eng.embed_f32_nchw(big, logits=True)
        eng.set_hw_sib_f16(True)
        on = eng.embed_f32_nchw(big, logits=True)
        eng.set_hw_sib_f16(False)
        after = eng.embed_f32_nchw(big, logits=True)
        for a, b in ((before, on), (before, after)):
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), mode


# ---------------------------------------------------------------------------------------------- 4. the setting's rules
@pytest.mark.parametrize("arch", SIBS)
def test_the_setting(eng0, blobs, blob_se, arch):
    eng = eng0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 23, *SIZE)).numpy()
    out = np.empty((3, 512), np.float32)

    def status():
        return eng.lib.reid_embed_f32_nchw_hw(eng.h, _p(x), 3, SIZE[0], SIZE[1], _p(out), None)

    eng.load_seres18(*blobs[arch])
    # with the setting at 0: today's refusals, word for word
    assert status() == -1
    assert eng.lib.reid_last_error().decode() == (
        "reid_embed_f32_nchw_hw: input size 96 x 72 runs seres18_ibn in precision mode 0 (exact fp32) only; loaded architecture "
        "%s, precision mode 0 (256 x 128 runs every architecture and mode)" % arch)
    eng.set_hw_f16(True)
    for sib, ema in ((0, 0), (1, 1)):
        eng.set_hw_siblings(bool(sib))
        eng.set_hw_ema(bool(ema))
        assert status() == -1
        assert eng.lib.reid_last_error().decode() == (
            "reid_embed_f32_nchw_hw: input size 96 x 72 with reid_ctx_set_hw_f16 1: loaded architecture %s; the fp16-storage any-size forward "
            "serves seres18_ibn only" % arch)
    eng.set_hw_f16(False)
    eng.set_hw_siblings(False)
    eng.set_hw_ema(False)
    if arch == "emares18_ibn":
        eng.set_hw_siblings(True)
        assert status() == -1 and "only cares18_ibn" in eng.lib.reid_last_error().decode()
        eng.set_hw_siblings(False)
    # bad values: REID_ERR_ARG, nothing changes
    for bad in (2, -1, 7):
        assert eng.lib.reid_ctx_set_hw_sib_f16(eng.h, bad) == -1 and "reid_ctx_set_hw_sib_f16" in eng.lib.reid_last_error().decode()
    assert status() == -1
    # 1: the same bits whatever the mode, hw_precision, hw_siblings, hw_ema and hw_f16
    eng.set_hw_sib_f16(True)
    seen = []
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        for v in (-1, 0, 2):
            eng.set_hw_precision(v)
            for sib, ema, f16 in ((0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)):
                eng.set_hw_siblings(bool(sib))
                eng.set_hw_ema(bool(ema))
                eng.set_hw_f16(bool(f16))
                assert status() == 0, (mode, v, sib, ema, f16, eng.lib.reid_last_error())
                seen.append(out.copy())
                assert eng.hw_precision == v and eng.precision == mode
    assert all(np.array_equal(_bits(s), _bits(seen[0])) for s in seen)
    # the other settings govern again at 0
    eng.set_precision(0)
    eng.set_hw_precision(0)
    eng.set_hw_f16(False)
    eng.set_hw_siblings(True)
    eng.set_hw_ema(True)
    eng.set_hw_sib_f16(False)
    exact = eng.embed_f32_nchw(x)
    assert not np.array_equal(_bits(exact), _bits(seen[0]))
    eng.set_hw_siblings(False)
    eng.set_hw_ema(False)
    assert status() == -1
    # seres18_ibn is not affected
    eng.load_seres18(*blob_se)
    for f16 in (False, True):
        eng.set_hw_f16(f16)
        eng.set_hw_sib_f16(False)
        off = eng.embed_f32_nchw(x)
        eng.set_hw_sib_f16(True)
        assert np.array_equal(_bits(eng.embed_f32_nchw(x)), _bits(off)), f16
    assert eng.fault_bits() == 0


def test_a_refused_submit_leaves_the_pending_frame(eng0, blobs):
    eng = _load(eng0, blobs, "cares18_ibn")
    crops, size = synth.ragged_crops_u8(3, seed=6), (128, 64)
    want = eng.embed_ragged_u8(crops, size=size)
    for f16, word in ((False, "precision mode 0 (exact fp32) only"), (True, "serves seres18_ibn only")):
        eng.set_hw_f16(False)
        eng.set_hw_sib_f16(True)
        eng.frame_submit_hw(1, crops, size)
        eng.frame_cost(1, want_emb=True)
        eng.set_hw_sib_f16(False)                                             # at 0: today's refusals, with and without hw_f16
        eng.set_hw_f16(f16)
        slab, offs, hw, n = eng._frame_pack(1, crops)
        assert eng.lib.reid_frame_submit_hw(eng.h, 1, _p(slab), _p(offs), _p(hw), n, size[0], size[1], None) == -1
        msg = eng.lib.reid_last_error().decode()
        assert "cares18_ibn" in msg and word in msg, msg
        assert np.array_equal(_bits(eng.frame_fetch(1)[0]), _bits(want)), "a refused submit touched the pending frame"


@pytest.mark.parametrize("arch", SIBS)
def test_plugin_objects(eng0, blobs, sds, fxs, arch):
    from reid_amd import inference_utils, reid_inference
    from reid_amd.backbone import cares18_ibn, emares18_ibn
    from reid_amd.extractor import Extractor
    eng = _load(eng0, blobs, arch)
    p, h, w, n, x = _case_input(fxs[arch], 1)
    crops = synth.ragged_crops_u8(4, seed=5)
    want = eng.embed_f32_nchw(x.numpy())
    want_crops = eng.embed_ragged_u8(crops, size=(h, w))
    want_desc = eng.descriptor_f32_nchw(x.numpy())
    eng.set_hw_sib_f16(False)

    def untouched():
        return eng.hw_sib_f16 is False and eng.hw_f16 is False and eng.hw_precision == -1 and not eng.hw_siblings and not eng.hw_ema

    model = (cares18_ibn if arch == "cares18_ibn" else emares18_ibn)(num_classes=751, loss="triplet", hw_sib_f16=True)
    model.load_state_dict(sds[arch])
    for mode in (0, 2):
        eng.set_precision(mode)
        got = np.asarray(model(x.numpy()))
        assert eng.precision == mode and untouched()
        assert np.array_equal(_bits(got), _bits(want))
    eng.set_precision(0)
    ext = Extractor(sds[arch], size=(w, h), hw_sib_f16=True)
    feats = ext(crops)
    assert untouched() and np.array_equal(_bits(feats), _bits(want_crops))
    eng.load_seres18(*blobs[arch])
    kw = {"hw_ema": True} if arch == "emares18_ibn" else {}
    d = DevArray(eng, (n, 1263))
    try:
        reid_inference.inference_efficient(eng, x.numpy(), d.ptr, arch=HW_ARCH[arch], hw_sib_f16=True, **kw)
        assert np.array_equal(_bits(d.numpy()), _bits(want_desc)) and untouched()
    finally:
        d.free()
    assert np.array_equal(_bits(inference_utils.extract_descriptors(x.numpy(), hw_sib_f16=True)), _bits(want_desc)) and untouched()


# ---------------------------------------------------------------------------------------------- 5. without the library
_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
x = np.zeros((1, 3, 96, 72), np.float32)
ok = True
for make, kw in ((synth.cares18_state_dict, "set_hw_siblings"), (synth.emares18_state_dict, "set_hw_ema")):
    eng.load_seres18(*weights.pack_seres18(make(0))[:2])
    getattr(eng, kw)(True)
    eng.set_hw_precision(0)
    before = eng.embed_f32_nchw(x)
    eng.set_hw_sib_f16(True)
    for call in (lambda: eng.embed_f32_nchw(x), lambda: eng.frame_submit_hw(0, [np.zeros((40, 20, 3), np.uint8)], (128, 64))):
        try:
            call()
            print("RAN")
            ok = False
        except _ffi.ReidHipError as e:
            print("RAISED", e.status, e)
            ok = ok and e.status == -3 and "libreid_hip_anysize_sib_f16.so" in str(e)
    eng.set_hw_sib_f16(False)
    ok = ok and np.array_equal(eng.embed_f32_nchw(x), before)           # the siblings in fp32, before and after
    getattr(eng, kw)(False)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
eng.set_hw_f16(True)
eng.set_hw_sib_f16(True)
se = eng.embed_f32_nchw(x)                                              # seres18_ibn with hw_f16 needs nothing of the new file
ok = ok and se.shape == (1, 512) and bool(np.isfinite(se).all()) and eng.fault_bits() == 0
sys.exit(0 if ok else 3)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_anysize_sib_f16.so, loaded through REID_HIP_LIB in a fresh child process: a sibling at
    another size under the setting is REID_ERR_STATE naming the file, the frame submit too; seres18_ibn with hw_f16 and the siblings in
    fp32 run."""
    lib = "libreid_hip_anysize_sib_f16.so"
    shutil.copytree(os.path.join(ROOT, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(ROOT, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    res = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
