"""The evaluation chain from uint8 images on the MI355X (pytest -m gpu): the two kernels of libreid_hip_pil_resize.so through the launcher
the entries call, bit for bit against tests/pil_resize_ref.py (itself held to Pillow and torch by tests/test_pil_resize_host.py and
tests/golden/pil_resize.npz); reid_descriptor_images_u8 and reid_swin_descriptor_images_u8 bit for bit against the float entries on the
oracle's floats; the refusals; and evaluate_reid on uint8 lists against evaluate_reid on the oracle's floats.

Everything here is an equality: integer arithmetic has one answer and the normalised float is a table lookup, so there is no bound to
derive."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

VIEWS = 6
NC = 24                                           # a small classifier: the descriptor's width is NC + 512 / NC + 96
CUSTOM_MS = (0.5, 0.4, 0.3, 0.25, 0.2, 0.3)
# 6 ragged images of the ResNet test, 3 of the Swin test, 12 + 6 of the chain: up- and down-scaling, mixed, one axis only, Market's size
SIX = ((128, 64), (300, 117), (90, 200), (64, 32), (257, 129), (256, 64))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _images(sizes, salt=0):
    return [ref.formula_image(h, w, salt + i) for i, (h, w) in enumerate(sizes)]


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
    return np.load(os.path.join(golden_dir, "pil_resize.npz"))


@pytest.fixture(scope="module")
def sources():
    return _images(ref.SOURCES)


@pytest.fixture(scope="module")
def oracle_u8(sources):
    """The oracle's resized images of the 13 sources at the three output sizes, computed once."""
    return {size: np.stack([ref.resize_u8(s, *size) for s in sources]) for size in ref.OUT_SIZES}


@pytest.fixture(scope="module")
def se_blobs():
    sd = synth.seres18_state_dict(0, num_class=NC)
    return {"cls": weights.pack_seres18(sd)[:2], "nocls": weights.pack_seres18({k: v for k, v in sd.items() if not k.startswith("classifier")})[:2]}


@pytest.fixture(scope="module")
def swin_blobs():
    out = {v: weights.pack_swin(synth.swin_state_dict(0, num_class=NC, views=VIEWS, version=v))[:2] for v in ("v1", "v2")}
    out["nocls"] = weights.pack_swin({k: v for k, v in synth.swin_state_dict(0, num_class=NC, views=VIEWS).items()
                                      if not k.startswith("mlp_head")})[:2]
    return out


def _load_se(eng, blobs, key, mode, chunk=1024):
    eng.set_side_index(None)
    eng.set_precision(0)
    eng.load_seres18(*blobs[key])
    eng.set_precision(mode)
    eng.set_chunk(chunk)


def _load_swin(eng, blobs, key, mode, chunk=1024):
    eng.set_side_index(None)
    eng.set_precision(0)
    eng.load_swin(*blobs[key])
    eng.set_precision(mode)
    eng.set_chunk(chunk)


# ----------------------------------------------------------------------------- 1. the harness
@pytest.mark.parametrize("size", ref.OUT_SIZES, ids=lambda s: "%dx%d" % s)
def test_harness_equals_the_oracle_on_the_thirteen_sources(eng, sources, oracle_u8, size):
    """One ragged call over the 13 sources (1 x 1 to 1031 x 517: up- and down-scaling, mixed, one axis only, identity): the resized uint8
    image and the normalised floats equal the oracle's bit for bit; every float was written (the harness fills with NaN)."""
    u8, f32 = eng.debug_pil_resize(sources, size)
    assert u8.shape == (13,) + size + (3,) and f32.shape == (13, 3) + size and np.isfinite(f32).all()
    for i in range(13):
        assert np.array_equal(u8[i], oracle_u8[size][i]), "source %r: %d bytes differ" % (ref.SOURCES[i], (u8[i] != oracle_u8[size][i]).sum())
        assert np.array_equal(_bits(f32[i]), _bits(ref.to_float(oracle_u8[size][i]))), "source %r" % (ref.SOURCES[i],)
    _, f32_only = eng.debug_pil_resize(sources, size, want_u8=False)                       # u8_out == NULL: the floats alone
    assert np.array_equal(_bits(f32_only), _bits(f32))


def test_harness_equals_pillow_on_the_small_fixture_cases(eng, fx):
    """The fixture's small cases at their own output sizes (16x8, 24x24, 32x16), grouped per size into ragged calls: Pillow's bytes and
    torch's floats themselves."""
    groups = {}
    for i in range(int(fx["n_small"])):
        groups.setdefault(tuple(int(v) for v in fx["out_%d" % i]), []).append(i)
    assert len(groups) == 3
    for size, idx in groups.items():
        u8, f32 = eng.debug_pil_resize([fx["src_%d" % i] for i in idx], size)
        for j, i in enumerate(idx):
            assert np.array_equal(u8[j], fx["u8_%d" % i]), "case %d" % i
            assert np.array_equal(_bits(f32[j]), _bits(fx["f32_%d" % i])), "case %d" % i
    _, f32 = eng.debug_pil_resize([fx["src_0"]], fx["out_0"], mean_std=fx["custom_ms"])
    assert np.array_equal(_bits(f32[0]), _bits(fx["f32_custom_0"]))


def test_harness_with_other_mean_std_shared_bytes_and_descending_offsets(eng, sources, oracle_u8):
    """Custom mean / std on the 13 sources; then four items over three images of one buffer, their offsets in descending order and two
    items pointing at the same source bytes."""
    size = (256, 128)
    u8, f32 = eng.debug_pil_resize(sources, size, mean_std=CUSTOM_MS)
    assert np.array_equal(u8, oracle_u8[size])
    assert np.array_equal(_bits(f32), _bits(np.stack([ref.to_float(o, CUSTOM_MS) for o in oracle_u8[size]])))
    assert not np.array_equal(_bits(f32), _bits(np.stack([ref.to_float(o) for o in oracle_u8[size]])))
    pick = [sources[2], sources[5], sources[7]]                                    # 300 x 117, 90 x 200, 2 x 3
    starts = np.cumsum([0] + [p.size for p in pick])
    packed = np.concatenate([p.reshape(-1) for p in pick])
    order = [2, 1, 0, 1]
    offsets = np.array([starts[i] for i in order], np.int64)
    hw = np.array([pick[i].shape[:2] for i in order], np.int32)
    assert (np.diff(offsets[:3]) < 0).all() and offsets[1] == offsets[3]
    for sz in ((448, 224), (224, 224)):
        u8, f32 = eng.debug_pil_resize(None, sz, packed=packed, offsets=offsets, hw=hw)
        for j, i in enumerate(order):
            want = oracle_u8[sz][(2, 5, 7)[i]]
            assert np.array_equal(u8[j], want), (sz, j)
            assert np.array_equal(_bits(f32[j]), _bits(ref.to_float(want))), (sz, j)
    # sizes the entries never use: one output pixel, a prime size, the widest the harness takes
    for sz in ((1, 1), (37, 1024), (7, 5)):
        u8, f32 = eng.debug_pil_resize(pick, sz)
        for j, p in enumerate(pick):
            want = ref.resize_u8(p, *sz)
            assert np.array_equal(u8[j], want) and np.array_equal(_bits(f32[j]), _bits(ref.to_float(want))), (sz, j)


# ----------------------------------------------------------------------------- 2. the ResNet entry
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resnet_entry_equals_the_float_entry_on_oracle_floats(eng, se_blobs, mode):
    """reid_descriptor_images_u8 against reid_descriptor_f32_nchw on tests/pil_resize_ref.preprocess of the same 6 ragged images, in
    passes of 4 and 2, with and without the mirrored view: the same bits in every arithmetic mode."""
    images = _images(SIX, 40)
    pre = ref.preprocess(images, 256, 128)
    _load_se(eng, se_blobs, "cls", mode, chunk=4)
    try:
        for tta in (False, True):
            want = eng.descriptor_f32_nchw(pre, flip_tta=tta)
            got = eng.descriptor_images_u8(images, flip_tta=tta)
            assert got.shape == (6, 512 + NC) and np.isfinite(got).all()
            assert np.array_equal(_bits(got), _bits(want)), "mode %d tta %d: %d values differ" % (mode, tta, (_bits(got) != _bits(want)).sum())
        assert not np.array_equal(got[0], got[1])                                  # six images gave six descriptors
        cams = np.array([5, 0, 2, 2, 1, 4], np.int32)                             # camera bias: n indices serve both views of an image
        eng.set_side_index(np.concatenate([cams, cams]))
        want = eng.descriptor_f32_nchw(pre, flip_tta=True)                         # the float entry takes them per view: model(x, cam.repeat(2))
        eng.set_side_index(cams)
        sided = eng.descriptor_images_u8(images, flip_tta=True)
        assert np.array_equal(_bits(sided), _bits(want)) and not np.array_equal(sided, got)
        assert np.array_equal(_bits(eng.descriptor_images_u8(images, flip_tta=True)), _bits(got))          # nothing stayed pending
        eng.set_side_index(cams[:5])
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.descriptor_images_u8(images)
        assert ei.value.status == -1 and "side ind" in str(ei.value)
        if mode == 0:
            got = eng.descriptor_images_u8(images, flip_tta=True, mean_std=CUSTOM_MS)
            want = eng.descriptor_f32_nchw(ref.preprocess(images, 256, 128, CUSTOM_MS), flip_tta=True)
            assert np.array_equal(_bits(got), _bits(want))
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)


# ----------------------------------------------------------------------------- 3. the Swin entry
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_swin_entry_equals_the_float_entry_on_oracle_floats(eng, swin_blobs, version, mode):
    """reid_swin_descriptor_images_u8 against reid_swin_descriptor_f32_nchw on the oracle's floats: 3 ragged images in passes of 2 and 1,
    at 448 x 224 and 224 x 224, with and without pending side indices (which serve both views), mirrored view on and off."""
    images = _images(SIX[:3], 50)
    idx = np.array([5, 0, 2], np.int32)
    _load_swin(eng, swin_blobs, version, mode, chunk=2)
    try:
        for size in ((448, 224), (224, 224)):
            pre = ref.preprocess(images, *size)
            rows = {}
            for side in (None, idx):
                for tta in ((True, False) if side is None else (True,)):
                    eng.set_side_index(side)
                    want = eng.swin_descriptor_f32_nchw(pre, flip_tta=tta)
                    eng.set_side_index(side)
                    got = eng.swin_descriptor_images_u8(images, size=size, flip_tta=tta)
                    assert got.shape == (3, NC + 96) and np.isfinite(got).all()
                    assert np.array_equal(_bits(got), _bits(want)), (version, mode, size, side is not None, tta)
                    rows[side is not None, tta] = got
            assert not np.array_equal(rows[False, True], rows[True, True])        # the side indices did reach the forward
    finally:
        eng.set_side_index(None)
        eng.set_precision(0)
        eng.set_chunk(1024)


# ----------------------------------------------------------------------------- 4. refusals
def _raw(eng, name, hw, nbytes, n=None, size=None, out_floats=4096):
    """The C entry itself on a zeroed buffer of nbytes: -> status."""
    packed = np.zeros(max(nbytes, 1), np.uint8)
    hw = np.asarray(hw, np.int32).reshape(-1, 2)
    offs = np.zeros(len(hw), np.int64)
    out = np.zeros(out_floats, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = len(hw) if n is None else n
    if name == "swin":
        return eng.lib.reid_swin_descriptor_images_u8(eng.h, p(packed), p(offs), p(hw), n, size[0], size[1], None, 1, p(out))
    return eng.lib.reid_descriptor_images_u8(eng.h, p(packed), p(offs), p(hw), n, None, 1, p(out))


def test_refusals_come_from_the_host(eng, se_blobs, swin_blobs):
    """include/reid_hip.h: weights without a classifier REID_ERR_STATE (-3); an image without pixels, a size that is no multiple of 224
    and a source over the declared limit REID_ERR_ARG (-1), the latter naming the limit; n == 0 a no-op that leaves nothing pending.
    None of them touches the fault word, and the next call works."""
    from reid_amd.engine import Engine
    lim = Engine.PIL_MAX_SIDE
    images = _images(SIX[:2], 60)
    _load_se(eng, se_blobs, "cls", 0)
    _load_swin(eng, swin_blobs, "v1", 0)
    want_se, want_sw = eng.descriptor_images_u8(images), eng.swin_descriptor_images_u8(images)
    for name, size in (("se", None), ("swin", (448, 224))):
        assert _raw(eng, name, [[0, 5]], 16, size=size) == -1                                 # no pixels
        assert _raw(eng, name, [[4, 5], [3, 0]], 60, size=size) == -1
        assert _raw(eng, name, [[lim + 1, 1]], (lim + 1) * 3, size=size) == -1                # over the limit, either side
        assert str(lim).encode() in eng.lib.reid_last_error()
        assert _raw(eng, name, [[1, lim + 1]], (lim + 1) * 3, size=size) == -1
        assert _raw(eng, name, [[lim, 1]], lim * 3, size=size) == 0                           # the limit itself is accepted
        eng.set_side_index(np.array([1, 1], np.int32))
        assert _raw(eng, name, [[4, 5]], 60, n=0, size=size) == 0                             # n == 0: OK, and nothing stays pending
    assert _raw(eng, "swin", [[4, 5]], 60, size=(448, 200)) == -1
    assert _raw(eng, "swin", [[4, 5]], 60, size=(200, 224)) == -1
    assert _raw(eng, "swin", [[4, 5]], 60, size=(0, 224)) == -1
    assert eng.fault_bits() == 0
    assert np.array_equal(_bits(eng.descriptor_images_u8(images)), _bits(want_se))
    assert np.array_equal(_bits(eng.swin_descriptor_images_u8(images)), _bits(want_sw))      # two images: pending indices would change it
    eng.set_side_index(np.array([0, 1, 2], np.int32))                                         # 3 side indices for 2 images
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.swin_descriptor_images_u8(images)
    assert ei.value.status == -1 and "side ind" in str(ei.value)
    assert np.array_equal(_bits(eng.swin_descriptor_images_u8(images)), _bits(want_sw))
    _load_se(eng, se_blobs, "nocls", 0)
    _load_swin(eng, swin_blobs, "nocls", 0)
    for name, size in (("se", None), ("swin", (448, 224))):
        assert _raw(eng, name, [[4, 5]], 60, size=size) == -3
        assert b"no classifier" in eng.lib.reid_last_error()
    fresh = Engine(0)                                                                         # a context without any weights
    try:
        assert _raw(fresh, "se", [[4, 5]], 60) == -3
        assert _raw(fresh, "swin", [[4, 5]], 60, size=(448, 224)) == -3
        assert fresh.fault_bits() == 0
    finally:
        fresh.close()
    assert eng.fault_bits() == 0


def test_a_fault_word_that_predates_the_call_survives_it(eng, se_blobs, swin_blobs):
    """The sticky fault word (here bit 1: an activation f16 cannot hold in precision 2, raised by reid_conv2d_nhwc): both entries and
    the harness return REID_ERR_STATE without touching it; after clear_fault they work."""
    images = _images(SIX[:2], 70)
    _load_se(eng, se_blobs, "cls", 0)
    _load_swin(eng, swin_blobs, "v1", 0)
    rng = np.random.default_rng(3)
    x = rng.normal(size=(3, 16, 8, 512)).astype(np.float32)
    wt = (rng.normal(size=(512, 3, 3, 512)) / np.sqrt(9 * 512)).astype(np.float32)
    x[0, 0, 0, 0] = -1e5
    eng.set_precision(2)
    try:
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.conv2d_nhwc(x, wt, 1, 1)
        assert ei.value.status == -3 and eng.fault_bits() & 1
        eng.set_precision(0)
        for call in (lambda: eng.descriptor_images_u8(images), lambda: eng.swin_descriptor_images_u8(images),
                     lambda: eng.debug_pil_resize(images, (16, 8))):
            with pytest.raises(_ffi.ReidHipError) as ei:
                call()
            assert ei.value.status == -3 and eng.fault_bits() & 1
    finally:
        eng.set_precision(0)
        eng.clear_fault()
    assert eng.fault_bits() == 0
    assert np.isfinite(eng.descriptor_images_u8(images)).all() and np.isfinite(eng.swin_descriptor_images_u8(images)).all()


# ----------------------------------------------------------------------------- 5. the chain
CHAIN = ((128, 64), (300, 117), (90, 200), (64, 32), (257, 129), (256, 64), (100, 128), (140, 70), (256, 128), (77, 41), (31, 90), (200, 50))


@pytest.mark.parametrize("arch", ["seres18", "swin"])
def test_chain_on_uint8_lists_equals_the_chain_on_oracle_floats(eng, se_blobs, swin_blobs, arch):
    """evaluate_reid on 12 gallery and 6 query uint8 images of mixed sizes against evaluate_reid on the oracle's floats of the same images,
    with a fixed cluster_fn: the descriptors, the CMC curve and mAP are equal bit for bit (the ResNet family; a Swin at 448 x 224 with
    use_side)."""
    from reid_amd import reid_inference
    g_img, q_img = _images(CHAIN, 80), _images(CHAIN[:6], 200)
    gl = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3], np.int64)
    gc = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2], np.int64)
    gs = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1], np.int64)
    ql, qc, qs = np.array([1, 2, 3, 1, 2, 3], np.int64), np.array([3, 3, 3, 4, 4, 4], np.int64), np.zeros(6, np.int64)
    labels = np.concatenate([gl, ql])
    kw = dict(cluster_fn=lambda d: labels, verbose=False, engine=eng, k1=4, k2=2)
    if arch == "swin":
        _load_swin(eng, swin_blobs, "v1", 0)
        size = (448, 224)
        kw.update(arch="swin", use_side=True)
    else:
        _load_se(eng, se_blobs, "cls", 0)
        size = (256, 128)
    t_u8, t_f32 = {}, {}
    u8_kw = dict(kw, size=size) if arch == "swin" else kw
    cmc_u8, map_u8 = reid_inference.evaluate_reid(g_img, gl, gc, gs, q_img, ql, qc, qs, taps=t_u8, **u8_kw)
    cmc_f, map_f = reid_inference.evaluate_reid(ref.preprocess(g_img, *size), gl, gc, gs, ref.preprocess(q_img, *size), ql, qc, qs, taps=t_f32, **kw)
    assert t_u8["desc"].shape == (18, NC + (96 if arch == "swin" else 512)) and np.isfinite(t_u8["desc"]).all()
    assert np.array_equal(_bits(t_u8["desc"]), _bits(t_f32["desc"]))
    assert np.array_equal(_bits(cmc_u8), _bits(cmc_f)) and map_u8 == map_f
    assert len({d.tobytes() for d in t_u8["desc"]}) == 18                          # eighteen images, eighteen descriptors
