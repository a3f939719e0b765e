"""Host side of the Swin descriptor entry points (no GPU): the new library's kernel list and independence, the declared / bound /
exported surface, the Python argument checks up to the first device call, and the float64 oracle of the descriptor kernel against the
reference's own numbers (tests/golden/swin_eval.npz), with one mutation per rule of the descriptor."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, reid_inference
from reid_amd.backbone import SwinT, swin_t
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_eval_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_swin_eval.so")
ENTRIES = ("reid_swin_descriptor_f32_nchw", "reid_swin_descriptor_f32_nchw_dev", "reid_swin_descriptor_ragged_u8")
HARNESSES = ("reid_debug_swin_conv1_mirror", "reid_debug_swin_crop_front_mirror", "reid_debug_swin_descriptor")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "swin_eval.npz"))


def test_swin_eval_library_kernels_match_their_list(built, golden_dir):
    """The three kernels live in a library of their own that libreid_hip.so opens from its own directory on the first descriptor call:
    the kernel list equals tests/golden/kernels_swin_eval.json by name, no kernel has scratch, the product library does not name the
    file among what it needs, and it loads on its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_swin_eval.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 3
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["lds"] % 16 == 0 for v in got.values())          # nothing static in front of the descriptor kernel's dynamic LDS
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_swin_eval" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own                            # ... and it needs nothing of the product library
    lib = ctypes.CDLL(LIB)
    for sym in ("swin_eval_conv1_mirror", "swin_eval_crop_front_mirror", "swin_eval_descriptor", "swin_eval_max_classes"):
        assert hasattr(lib, sym)
    assert lib.swin_eval_max_classes() == 4096


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for sym in ENTRIES:
        assert sym + "(" in hdr and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    for sym in HARNESSES:
        assert sym + "(" in dbg_hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), sym)
    for name in ("swin_descriptor_f32_nchw", "swin_descriptor_dev", "swin_descriptor_ragged_u8", "debug_swin_descriptor"):
        assert callable(getattr(Engine, name))
    assert callable(getattr(SwinT, "descriptor"))


class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    swin_dim, swin_num_class, embed_dim, num_class = 96, 751, 512, 751
    _swin_crop_args = staticmethod(Engine._swin_crop_args)          # the engine's own host-side helpers: no device behind them
    _pack_ragged = staticmethod(Engine._pack_ragged)
    _swin_descriptor_width = Engine._swin_descriptor_width

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_python_argument_checks_raise_before_any_device_call():
    x = np.zeros((2, 3, 448, 224), np.float32)
    eng = _NoDevice()
    with pytest.raises(ValueError, match="224"):
        Engine.swin_descriptor_f32_nchw(eng, np.zeros((2, 3, 256, 128), np.float32))
    with pytest.raises(ValueError, match="224"):
        Engine.swin_descriptor_dev(eng, 1, 2, 448, 200, True, 1)
    with pytest.raises(ValueError):
        Engine.swin_descriptor_dev(eng, 0, 2, 448, 224, True, 1)
    with pytest.raises(ValueError, match="224"):
        Engine.swin_descriptor_ragged_u8(eng, [np.zeros((4, 4, 3), np.uint8)], size=(448, 200))
    with pytest.raises(ValueError):
        Engine.swin_descriptor_ragged_u8(eng, [np.zeros((4, 4, 3), np.uint8)], mean_std=[0.5] * 5)
    nocls = _NoDevice()
    nocls.swin_num_class = 0
    with pytest.raises(ValueError, match="classifier"):
        Engine.swin_descriptor_f32_nchw(nocls, x)
    m = swin_t(num_classes=5, camera=6)
    with pytest.raises(ValueError, match="224"):
        m.descriptor(np.zeros((1, 3, 256, 128), np.float32))
    with pytest.raises(ValueError):
        m.descriptor(x, view_index=[0])                              # one index per image
    with pytest.raises(ValueError, match="view_index"):
        m.descriptor(x, view_index=[0, 6])                           # outside the table of 6 views
    with pytest.raises(AttributeError):
        swin_t(num_classes=5).descriptor(x, view_index=[0, 1])       # built without camera / sequence, as model(x, view_index)
    # reid_inference: arch, shapes, side information
    with pytest.raises(ValueError, match="arch"):
        reid_inference.inference_efficient(eng, x, 1, arch="vit")
    with pytest.raises(ValueError, match="224"):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 256, 128), np.float32), 1, arch="swin")
    with pytest.raises(ValueError, match="256"):
        reid_inference.inference_efficient(eng, x, 1)                # the default stays the ResNet's 256 x 128
    with pytest.raises(ValueError, match="view_index"):
        reid_inference.inference_efficient(eng, x, 1, arch="swin", view_index=[0])
    with pytest.raises(ValueError, match="view_index"):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 256, 128), np.float32), 1, view_index=[0, 1])
    with pytest.raises(ValueError, match="classifier"):
        reid_inference.inference_efficient(nocls, x, 1, arch="swin")
    lab = np.zeros(2, np.int64)
    with pytest.raises(ValueError, match="use_side"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, use_side=True)
    with pytest.raises(ValueError, match="arch"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, arch="osnet")
    with pytest.raises(ValueError, match="224"):
        reid_inference.evaluate_reid(np.zeros((2, 3, 256, 128), np.float32), lab, lab, lab, x, lab, lab, lab, engine=eng, arch="swin")


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_oracle_reproduces_the_reference_descriptors(fx, version):
    """tests/swin_eval_ref.py on the fixture's x_norm / logits blocks gives the fixture's descriptors (fp32 blocks: to the reference's own
    fp32 noise), and descriptor64 - which runs the classifier itself - agrees with the reference's logits."""
    from reid_amd import synth
    tol = 20 * float(fx["ref_noise_" + version])
    for tag in ("a4", "a3"):
        b = {k: fx["%s_%s_%s" % (tag, k, version)] for k in ("xn1", "xn2", "lg1", "lg2", "tta", "plain", "mirror")}
        np.testing.assert_allclose(ref.descriptor_from_parts(b["lg1"], b["xn1"], b["lg2"], b["xn2"]), b["tta"], rtol=0, atol=tol)
        np.testing.assert_allclose(ref.descriptor_from_parts(b["lg1"], b["xn1"]), b["plain"], rtol=0, atol=tol)
        np.testing.assert_allclose(ref.descriptor_from_parts(b["lg2"], b["xn2"]), b["mirror"], rtol=0, atol=tol)
        np.testing.assert_allclose(b["tta"], fx["%s_tta_f64_%s" % (tag, version)], rtol=0, atol=1.01 * float(fx["ref_noise_" + version]) if tag == "a4" else tol)
        cls_w = synth.swin_state_dict(0, views=int(fx["views"]), version=version)["mlp_head.0.weight"]
        got, bound = ref.descriptor64(b["xn1"], b["xn2"], cls_w)
        np.testing.assert_allclose(got, b["tta"], rtol=0, atol=tol)
        assert bound.shape == got.shape and (bound > 0).all() and bound.max() < float(fx["tta_effect_" + version]) / 100


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_each_rule_of_the_descriptor_is_held_by_the_bar(fx, version):
    """One mutation per rule, each shown to leave the bar of the GPU test against the reference (min(tta_effect, side_effect) / 16) by
    the stored effect sizes: the embedding part first, no final renormalisation, the mirrored view equal to the plain one - and the side
    indices dropped."""
    bar = min(float(fx["tta_effect_" + version]), float(fx["side_effect_" + version])) / 16
    assert float(fx["ref_noise_" + version]) * 100 < bar
    b = {k: fx["a4_%s_%s" % (k, version)].astype(np.float64) for k in ("xn1", "xn2", "lg1", "lg2")}
    want = fx["a4_tta_f64_" + version]
    nc = b["lg1"].shape[1]
    good = ref.descriptor_from_parts(b["lg1"], b["xn1"], b["lg2"], b["xn2"])
    assert np.abs(good - want).max() < bar / 100

    def off(d):
        return float(np.abs(d - want).max())
    swapped = np.concatenate([good[:, nc:], good[:, :nc]], 1)                                  # [x_norm | logits], the ResNet's order
    assert off(swapped) > 100 * bar
    d1, d2 = ref.descriptor_from_parts(b["lg1"], b["xn1"]), ref.descriptor_from_parts(b["lg2"], b["xn2"])
    assert off((d1 + d2) / 2.0) > 100 * bar                                                     # no final renormalisation
    same_view = ref.descriptor_from_parts(b["lg1"], b["xn1"], b["lg1"], b["xn1"])               # the mirror forgotten
    assert off(same_view) == pytest.approx(float(fx["tta_effect_" + version]), rel=1e-3) and off(same_view) > 15 * bar
    assert float(fx["side_effect_" + version]) > 15 * bar                                       # the side indices forgotten
