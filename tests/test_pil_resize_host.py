"""Host side of the *_images_u8 entry points (no GPU): the numpy oracle of Pillow's 8-bit bilinear resize (tests/pil_resize_ref.py)
against what Pillow and torch wrote into tests/golden/pil_resize.npz, one mutation per rule of that arithmetic, the side library's
coefficient function, kernel list and independence, the declared / bound / exported surface, and the Python argument checks up to the
first device call."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, reid_inference
from reid_amd import inference_utils
from reid_amd.backbone import SwinT, swin_t
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_pil_resize.so")
ENTRIES = ("reid_descriptor_images_u8", "reid_swin_descriptor_images_u8")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "pil_resize.npz"))


def _small(fx):
    for i in range(int(fx["n_small"])):
        yield i, fx["src_%d" % i], tuple(int(v) for v in fx["out_%d" % i]), fx["u8_%d" % i], fx["f32_%d" % i]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. the oracle against the fixture
def test_oracle_equals_pillow_and_torch_on_the_small_cases(fx):
    """Every small case in full: the resized uint8 image equals Pillow's byte for byte, the normalised floats torch's bit for bit."""
    assert int(fx["n_small"]) >= 8
    for i, src, (oh, ow), u8, f32 in _small(fx):
        assert max(src.shape[:2]) <= 64
        got = ref.resize_u8(src, oh, ow)
        assert got.dtype == np.uint8 and np.array_equal(got, u8), "case %d: %d bytes differ" % (i, (got != u8).sum())
        assert np.array_equal(_bits(ref.to_float(got)), _bits(f32)), "case %d" % i
    ms = tuple(float(v) for v in fx["custom_ms"])
    assert np.array_equal(_bits(ref.to_float(fx["u8_0"], ms)), _bits(fx["f32_custom_0"]))
    assert np.array_equal(_bits(ref.norm_table()), _bits(fx["table"]))
    assert np.array_equal(_bits(ref.preprocess([fx["src_0"]], *fx["out_0"])[0]), _bits(fx["f32_0"]))


def test_oracle_equals_pillow_digests_on_the_large_cases(fx):
    """The 13 x 3 large cases (sources up to 1031 x 517 from the stated integer formula, outputs 256x128, 448x224, 224x224) by SHA-256."""
    hw, out, salt, sha = fx["large_hw"], fx["large_out"], fx["large_salt"], fx["large_sha"]
    assert [tuple(v) for v in hw[::3]] == list(ref.SOURCES) and [tuple(v) for v in out[:3]] == list(ref.OUT_SIZES) and len(sha) == 39
    edge = ref.formula_image(300, 117, 2)                       # saturated borders: rows and columns of 0 and of 255
    assert (edge[0, :-1] == 0).all() and (edge[:-1, 0] == 0).all() and (edge[-1] == 255).all() and (edge[:, -1] == 255).all()
    for (h, w), (oh, ow), s, want in zip(hw, out, salt, sha):
        src = ref.formula_image(int(h), int(w), int(s))
        got = hashlib.sha256(ref.resize_u8(src, int(oh), int(ow)).tobytes()).hexdigest()
        assert got == str(want), "%d x %d -> %d x %d" % (h, w, oh, ow)


def test_oracle_equals_pillow_live():
    """Where Pillow is importable: the same 39 cases against Image.resize itself."""
    Image = pytest.importorskip("PIL.Image")
    for si, (h, w) in enumerate(ref.SOURCES):
        src = ref.formula_image(h, w, si)
        for oh, ow in ref.OUT_SIZES:
            want = np.asarray(Image.fromarray(src, "RGB").resize((ow, oh), Image.BILINEAR))
            assert np.array_equal(ref.resize_u8(src, oh, ow), want), "%d x %d -> %d x %d" % (h, w, oh, ow)


# ---------------------------------------------------------------------------------------------- 2. one mutation per rule
@pytest.mark.parametrize("mutation", [dict(vertical_first=True), dict(round_between=False), dict(widen=False), dict(rounding=False),
                                      dict(renorm=False)], ids=lambda m: next(iter(m)))
def test_each_rule_is_held_by_the_fixture(fx, mutation):
    """The oracle with ONE rule of Resample.c broken - vertical pass first, no uint8 rounding between the passes, 2-tap sampling without
    the widened support, truncation instead of + (1 << 21), weights not renormalised at a clipped edge - disagrees with Pillow's output
    on at least one small case, while the unbroken oracle agrees on all."""
    wrong = [i for i, src, (oh, ow), u8, _ in _small(fx) if not np.array_equal(ref.resize_u8(src, oh, ow, **mutation), u8)]
    assert wrong, "the fixture cannot tell %r from Pillow" % (mutation,)


# ---------------------------------------------------------------------------------------------- 3. the side library
def test_side_library_coefficients_equal_the_oracle(built):
    """pil_resize_coeffs (host code of the side library, double without contraction) against the oracle's tables for every in from 1 to
    300 and 517, 1031, 2048, each to 128, 224, 256 and 448; every window stays inside the source and inside ksize."""
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    for size_in in list(range(1, 301)) + [517, 1031, 2048]:
        for size_out in (128, 224, 256, 448):
            ks = ctypes.c_int(-1)
            assert lib.pil_resize_coeffs(size_in, size_out, None, None, ctypes.byref(ks)) == 0
            k = np.full((size_out, ks.value), -7, np.int32)
            b = np.full((size_out, 2), -7, np.int32)
            assert lib.pil_resize_coeffs(size_in, size_out, k.ctypes.data_as(vp), b.ctypes.data_as(vp), ctypes.byref(ks)) == 0
            rk, rb, rks = ref.coeffs(size_in, size_out)
            assert rks == ks.value and np.array_equal(k, rk) and np.array_equal(b, rb), (size_in, size_out)
            assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= size_in).all() and (b[:, 1] <= ks.value).all()
    ks = ctypes.c_int()
    assert lib.pil_resize_coeffs(0, 8, None, None, ctypes.byref(ks)) != 0 and lib.pil_resize_coeffs(8, 0, None, None, ctypes.byref(ks)) != 0
    for ms in (ref.IMAGENET_MEAN_STD, (0.5, 0.4, 0.3, 0.25, 0.2, 0.3)):
        tab = np.zeros((3, 256), np.float32)
        lib.pil_resize_norm_table(np.asarray(ms, np.float32).ctypes.data_as(vp), tab.ctypes.data_as(vp))
        assert np.array_equal(_bits(tab), _bits(ref.norm_table(ms)))
    assert lib.pil_resize_max_side() == Engine.PIL_MAX_SIDE >= 2048 and lib.pil_resize_max_out() == 1024


def test_side_library_kernels_match_their_list(built, golden_dir):
    """The two kernels live in a library of their own: its kernel list equals tests/golden/kernels_pil_resize.json by name, no kernel
    has scratch, the product library does not name the file among what it needs, and it loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_pil_resize.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 2
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_pil_resize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own      # it needs nothing of the product library or its siblings
    lib = ctypes.CDLL(LIB)
    for sym in ("pil_resize_max_side", "pil_resize_max_out", "pil_resize_coeffs", "pil_resize_norm_table", "pil_resize_launch"):
        assert hasattr(lib, sym)


# ---------------------------------------------------------------------------------------------- 4. surface
def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for sym in ENTRIES:
        assert sym + "(" in hdr and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    assert "reid_debug_pil_resize(" in dbg_hdr and "reid_debug_pil_resize" in _ffi.DEBUG_EXPORTS
    assert hasattr(_ffi.debug_lib(), "reid_debug_pil_resize")
    import re
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M)) | set(re.findall(r"^const char\*\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert set(ENTRIES) <= declared and set(ENTRIES) <= set(_ffi.EXPORTS)
    for name in ("descriptor_images_u8", "swin_descriptor_images_u8", "debug_pil_resize"):
        assert callable(getattr(Engine, name))
    assert callable(getattr(SwinT, "descriptor_images"))


class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    swin_dim, swin_num_class, embed_dim, num_class = 96, 751, 512, 751
    PIL_MAX_SIDE = Engine.PIL_MAX_SIDE
    _swin_crop_args = staticmethod(Engine._swin_crop_args)          # the engine's own host-side helpers: no device behind them
    _pack_ragged = staticmethod(Engine._pack_ragged)
    _pack_images = classmethod(Engine._pack_images.__func__)
    _swin_descriptor_width = Engine._swin_descriptor_width

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_python_argument_checks_raise_before_any_device_call():
    eng = _NoDevice()
    ok = [np.zeros((4, 5, 3), np.uint8)]
    big = [np.zeros((Engine.PIL_MAX_SIDE + 1, 1, 3), np.uint8)]
    for images in ([np.zeros((4, 5), np.uint8)], [np.zeros((0, 5, 3), np.uint8)], [np.zeros((4, 5, 4), np.uint8)], big):
        with pytest.raises(ValueError):
            Engine.descriptor_images_u8(eng, images)
        with pytest.raises(ValueError):
            Engine.swin_descriptor_images_u8(eng, images)
        with pytest.raises(ValueError):
            Engine.debug_pil_resize(eng, images, (16, 8))
    with pytest.raises(ValueError, match="224"):
        Engine.swin_descriptor_images_u8(eng, ok, size=(448, 200))
    with pytest.raises(ValueError):
        Engine.swin_descriptor_images_u8(eng, ok, mean_std=[0.5] * 5)
    with pytest.raises(ValueError):
        Engine.descriptor_images_u8(eng, ok, mean_std=[0.5, 0.5, 0.5, 0.2, 0.0, 0.2])          # std must be positive
    nocls = _NoDevice()
    nocls.swin_num_class = nocls.num_class = 0
    with pytest.raises(ValueError, match="classifier"):
        Engine.swin_descriptor_images_u8(nocls, ok)
    with pytest.raises(ValueError, match="classifier"):
        Engine.descriptor_images_u8(nocls, ok)
    for size in ((0, 8), (8, 1025), 7):
        with pytest.raises(ValueError):
            Engine.debug_pil_resize(eng, ok, size)
    with pytest.raises(ValueError, match="leaves"):
        Engine.debug_pil_resize(eng, None, (8, 8), packed=np.zeros(59, np.uint8), offsets=[0], hw=[[4, 5]])
    m = swin_t(num_classes=5, camera=6)
    with pytest.raises(ValueError, match="224"):
        m.descriptor_images(ok, size=(256, 128))
    with pytest.raises(ValueError, match="uint8"):
        m.descriptor_images([np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(ValueError):
        m.descriptor_images(ok, view_index=[0, 1])                       # one index per image
    with pytest.raises(ValueError, match="view_index"):
        m.descriptor_images(ok, view_index=[6])                          # outside the table of 6 views
    with pytest.raises(AttributeError):
        swin_t(num_classes=5).descriptor_images(ok, view_index=[0])
    # reid_inference: uint8 sequences, their size argument, limits
    assert reid_inference.is_u8_images(ok) and reid_inference.is_u8_images(np.zeros((2, 4, 5, 3), np.uint8))
    assert not reid_inference.is_u8_images(np.zeros((2, 3, 256, 128), np.float32)) and not reid_inference.is_u8_images([])
    with pytest.raises(ValueError, match="256"):
        reid_inference.inference_efficient(eng, ok, 1, size=(448, 224))                      # the ResNet family is fixed at 256 x 128
    with pytest.raises(ValueError, match="224"):
        reid_inference.inference_efficient(eng, ok, 1, arch="swin", size=(448, 200))
    with pytest.raises(ValueError, match="uint8"):
        reid_inference.inference_efficient(eng, [np.zeros((4, 5), np.uint8)], 1)
    with pytest.raises(ValueError, match="at most"):
        reid_inference.inference_efficient(eng, big, 1, arch="swin")
    with pytest.raises(ValueError, match="size"):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 448, 224), np.float32), 1, arch="swin", size=(448, 224))
    with pytest.raises(ValueError, match="view_index"):
        reid_inference.inference_efficient(eng, ok, 1, arch="swin", view_index=[0, 1])
    with pytest.raises(ValueError, match="view_index"):
        reid_inference.inference_efficient(eng, ok, 1, view_index=[0])
    with pytest.raises(ValueError, match="bs"):
        reid_inference.inference_efficient(eng, ok, 1, bs=0)
    lab = np.zeros(1, np.int64)
    with pytest.raises(ValueError, match="uint8"):
        reid_inference.evaluate_reid(ok, lab, lab, lab, [np.zeros((4, 5, 1), np.uint8)], lab, lab, lab, engine=eng)
    with pytest.raises(ValueError, match="256"):
        reid_inference.evaluate_reid(ok, lab, lab, lab, ok, lab, lab, lab, engine=eng, size=(224, 224))
    with pytest.raises(ValueError, match="size"):
        x = np.zeros((1, 3, 256, 128), np.float32)
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, size=(256, 128))
    with pytest.raises(ValueError, match="disagree"):
        reid_inference.evaluate_reid(ok + ok, lab, lab, lab, ok, lab, lab, lab, engine=eng)
    assert callable(inference_utils.extract_descriptors)
