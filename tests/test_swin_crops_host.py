"""Host side of the Swin uint8 entry points (no GPU): the fp32 restatement of the front end against float64, the new library's kernel
list and independence, and the Python surface up to the first device call."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, extractor, synth, weights
from reid_amd.backbone import SwinT, swin_t
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_crops_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_swin_crops.so")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("size,mean_std", [((224, 224), None), ((448, 224), ref.OTHER_MEAN_STD)], ids=["224x224-imagenet", "448x224-other"])
def test_preprocess_restatement_bounds_the_fp32_path(size, mean_std):
    """swin_crops_ref.preprocess (fp32, what the fused path must equal bit for bit) is within the derived bound of the float64
    restatement on every crop shape of the GPU test; the two are different computations; a crop already at the size is not resampled."""
    mean, std = (ref.IMAGENET_MEAN, ref.IMAGENET_STD) if mean_std is None else (mean_std[:3], mean_std[3:])
    _, crops, _ = ref.crop_set()
    worst = 0.0
    got_all = ref.preprocess(crops, size, mean, std)
    assert got_all.shape == (len(crops), 3) + size and got_all.dtype == np.float32
    for crop, got in zip(crops, got_all):
        want, b = ref.preprocess64(crop, size, mean, std)
        err = np.abs(got.transpose(1, 2, 0).astype(np.float64) - want)
        assert (err <= b).all(), crop.shape
        worst = max(worst, float((err / b).max()))
    assert worst > 0.0
    if size == (224, 224):
        ident = crops[4]
        assert ident.shape == (224, 224, 3)
        want = ((ident.astype(np.float32) / np.float32(255.0)) - mean) / std
        np.testing.assert_array_equal(got_all[4].transpose(1, 2, 0), want)


def test_front64_is_torch_conv_of_the_preprocessed_image():
    """The float64 restatement of the whole front end is torch's float64 conv2d (2x2, stride 2) of the float64 preprocessing."""
    import torch
    w, b = ref.conv_weights()
    _, crops, _ = ref.crop_set()
    for crop in (crops[1], crops[6]):
        x, _ = ref.preprocess64(crop)
        want = torch.nn.functional.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2),
                                          torch.from_numpy(b.astype(np.float64)), 2)[0].permute(1, 2, 0).numpy()
        got, bound = ref.front64(crop, w, b)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        assert got.shape == (112, 112, 12) and bound.shape == got.shape and (bound > 0).all()


def test_swin_crops_library_kernels_match_their_list(built, golden_dir):
    """The front kernel lives in a library of its own, libreid_hip_swin_crops.so, that libreid_hip.so opens from its own directory on the
    first crops call: its kernel list equals tests/golden/kernels_swin_crops.json by name, the kernel has no scratch, the product library
    does not name it among what it needs, and it loads on its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_swin_crops.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 1 and "swin_crop_front_kernel" in list(got)[0]
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_swin_crops" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own                            # ... and it needs nothing of the product library
    assert hasattr(ctypes.CDLL(LIB), "swin_crops_front")


def test_the_two_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for sym in ("reid_swin_embed_ragged_u8", "reid_swin_embed_frame_u8"):
        assert sym + "(" in hdr and sym in _ffi.EXPORTS and hasattr(lib, sym)
    for sym in ("reid_debug_swin_crop_front", "reid_debug_swin_conv1"):
        assert sym in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), sym)


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_extractor_recognises_a_swin_checkpoint_by_its_keys(version):
    """Through the packing step only (extractor.pack_checkpoint): no engine, no device."""
    sd = synth.swin_state_dict(0, num_class=5, version=version)
    assert weights.is_swin_state_dict(sd) and weights.is_swin_state_dict({"state_dict": {"module." + k: v for k, v in sd.items()}})
    arch, blob, manifest, info = extractor.pack_checkpoint(sd)
    want = weights.pack_swin(sd)
    assert arch == "swin" and info == want[2] and info["embed_dim"] == 96 and manifest == want[1]
    np.testing.assert_array_equal(blob, want[0])
    assert ("swin.version" in manifest) == (version == "v2")


def test_extractor_packs_a_resnet_checkpoint_as_before():
    sd = synth.seres18_state_dict(0, num_class=5)
    assert not weights.is_swin_state_dict(sd)
    arch, blob, manifest, info = extractor.pack_checkpoint(sd)
    want = weights.pack_seres18(sd)
    assert arch == "seres18" and manifest == want[1] and info == want[2]
    np.testing.assert_array_equal(blob, want[0])


def test_bad_sizes_raise_before_any_device_call():
    """SwinT has embed_crops / embed_frame; a size that is no multiple of 224 (out_h = 200) raises ValueError in Python - with no GPU in
    this test, anything that reached the engine would fail differently."""
    assert callable(getattr(SwinT, "embed_crops")) and callable(getattr(SwinT, "embed_frame"))
    crop = np.zeros((10, 10, 3), np.uint8)
    m = swin_t(num_classes=5)
    with pytest.raises(ValueError, match="224"):
        m.embed_crops([crop], size=(200, 224))
    with pytest.raises(ValueError, match="224"):
        m.embed_frame(crop, [[0, 0, 5, 5]], size=(224, 100))
    for bad in ((200, 224), (224, 0), (-224, 224), (224,)):
        with pytest.raises(ValueError):
            Engine._swin_crop_args(bad, None)
    for bad_ms in ([0.5] * 5, [0.5, 0.5, 0.5, 0.2, 0.0, 0.2], [0.5, 0.5, 0.5, 0.2, np.nan, 0.2]):
        with pytest.raises(ValueError):
            Engine._swin_crop_args((224, 224), bad_ms)
    assert Engine._swin_crop_args((448, 224), None) == (448, 224, None)
    h, w, ms = Engine._swin_crop_args((224, 448), ref.OTHER_MEAN_STD)
    assert (h, w) == (224, 448) and ms.dtype == np.float32 and ms.tolist() == ref.OTHER_MEAN_STD.tolist()
