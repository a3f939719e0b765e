"""Host side of the any-size ResNet18-IBN-SE forward (no GPU): the float64 restatement of its three kernel families (tests/anysize_ref.py)
against torch, one mutation per kernel that a subtly wrong version fails, the size and pass-size rules up to the first device call, the
side library's kernel list and independence, the declared / bound / exported surface, and the fixture's own shape."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from reid_amd import _ffi, engine as engine_mod, inference_utils, reid_inference, synth
from reid_amd.backbone import seres18_ibn, cares18_ibn
from reid_amd.engine import Engine
from reid_amd.extractor import Extractor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize.so")
ENTRIES = ("reid_embed_f32_nchw_hw", "reid_embed_f32_nchw_hw_dev", "reid_embed_ragged_u8_hw", "reid_descriptor_f32_nchw_hw",
           "reid_descriptor_f32_nchw_hw_dev", "reid_descriptor_images_u8_hw")
HARNESSES = ("reid_debug_any_norm", "reid_debug_any_se_tail", "reid_debug_any_gem")
SIDE_SYMBOLS = ("anysize_norm", "anysize_se_tail", "anysize_gem", "anysize_nchw_to_nhwc3", "anysize_resize_norm")
# (hw, c): below a wavefront, odd, no multiple of 64, the VeRi stage-1 map 56 x 67
SHAPES = ((8, 64), (30, 64), (15, 128), (108, 64), (3752, 64))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _data(hw, c, seed, n=3):
    rng = np.random.default_rng(seed)
    x = (rng.normal(0.3, 1.0, (n, hw, c)) * rng.uniform(0.5, 2.0, (1, 1, c))).astype(np.float32)
    return rng, x


def _nchw(x, h, w):
    n, hw, c = x.shape
    return torch.from_numpy(np.asarray(x, np.float64)).reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def _fact(hw):
    for h in range(int(hw ** 0.5), 0, -1):
        if hw % h == 0:
            return h, hw // h


# ---------------------------------------------------------------------------------------------- 1. the restatement against torch
@pytest.mark.parametrize("hw,c", SHAPES)
def test_instance_norm_restatement_equals_torch(hw, c):
    """relu(IBN(x)): the first half through torch's InstanceNorm2d(affine) in float64, the other half a folded BatchNorm; and the
    mutation - the SAMPLE variance (divisor hw - 1) - is outside the restatement's own error bound at every shape."""
    rng, x = _data(hw, c, 1)
    half = c // 2
    gamma, beta = rng.uniform(0.5, 1.5, half).astype(np.float32), rng.normal(0, 0.2, half).astype(np.float32)
    s, t = rng.uniform(0.5, 1.5, c - half).astype(np.float32), rng.normal(0, 0.2, c - half).astype(np.float32)
    h, w = _fact(hw)
    xt = _nchw(x, h, w)
    inorm = torch.nn.InstanceNorm2d(half, affine=True).double()
    with torch.no_grad():
        inorm.weight.copy_(torch.from_numpy(gamma.astype(np.float64)))
        inorm.bias.copy_(torch.from_numpy(beta.astype(np.float64)))
        a = inorm(xt[:, :half])
        b = xt[:, half:] * torch.from_numpy(s.astype(np.float64))[None, :, None, None] + torch.from_numpy(t.astype(np.float64))[None, :, None, None]
        want = torch.relu(torch.cat([a, b], 1)).permute(0, 2, 3, 1).reshape(x.shape).numpy()
    got, bound = ref.instance_norm(x, gamma, beta, half, s, t)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert (bound > 0).all() and bound.max() < 1e-4
    kept, _ = ref.instance_norm(x, gamma, beta, half)                    # BatchNorm half left alone
    assert np.array_equal(kept[:, :, half:], x[:, :, half:].astype(np.float64)) and np.array_equal(kept[:, :, :half], got[:, :, :half])
    wrong, _ = ref.instance_norm(x, gamma, beta, half, s, t, sample_variance=True)
    assert (np.abs(wrong - got) > 10 * bound).any(), "a sample variance would pass"


@pytest.mark.parametrize("hw,c", SHAPES)
def test_se_tail_restatement_equals_torch(hw, c):
    """SEBlock as the network builds it (AdaptiveAvgPool2d(1), two bias-free 1x1 convolutions, ReLU, sigmoid) + relu(gate * y + shortcut)
    in float64 torch; the mutation - an average over hw rounded up to a multiple of 64 - is outside the bound wherever hw % 64 != 0."""
    rng, y = _data(hw, c, 2)
    sc = rng.normal(0, 1, y.shape).astype(np.float32)
    mid = max(c // 16, 8)
    w1 = rng.normal(0, 1 / np.sqrt(c), (mid, c)).astype(np.float32)
    w2 = rng.normal(0, 1 / np.sqrt(mid), (c, mid)).astype(np.float32)
    h, w = _fact(hw)
    yt, st = _nchw(y, h, w), _nchw(sc, h, w)
    with torch.no_grad():
        pooled = F.adaptive_avg_pool2d(yt, 1)
        z = F.conv2d(torch.relu(F.conv2d(pooled, torch.from_numpy(w1.astype(np.float64))[:, :, None, None])),
                     torch.from_numpy(w2.astype(np.float64))[:, :, None, None])
        gate_t = torch.sigmoid(z)
        want = torch.relu(gate_t * yt + st).permute(0, 2, 3, 1).reshape(y.shape).numpy()
    got, gate, bound, gbound = ref.se_tail(y, sc, w1, np.ascontiguousarray(w2.T))
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(gate - gate_t.reshape(gate.shape).numpy()).max() < 1e-14
    assert bound.max() < 1e-4 and gbound.max() < 1e-5
    if hw % 64:
        wrong, wgate, _, _ = ref.se_tail(y, sc, w1, np.ascontiguousarray(w2.T), avg_over=(hw + 63) // 64 * 64)
        assert (np.abs(wgate - gate) > 10 * gbound).any() and (np.abs(wrong - got) > 10 * bound).any(), "a padded average would pass"


@pytest.mark.parametrize("p", [3.0, 2.6])
@pytest.mark.parametrize("hw,c", SHAPES)
def test_gem_restatement_equals_torch(hw, c, p):
    """GeM as the pooling layer states it - avg_pool2d(x.clamp(min=eps).pow(p), (H, W)).pow(1 / p) - then the BNNeck's folded affine; the
    mutation - no clamp - is outside the bound (negative inputs: NaN for a trained p, a different mean for p = 3)."""
    rng, x = _data(hw, c, 3)
    x[0, 0, :] = 0.0                                                     # exact zeros and negatives are what the clamp is for
    scale, shift = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.2, c).astype(np.float32)
    h, w = _fact(hw)
    xt = _nchw(x, h, w)
    with torch.no_grad():
        g_t = F.avg_pool2d(xt.clamp(min=1e-6).pow(float(np.float32(p))), (h, w)).pow(1.0 / float(np.float32(p))).reshape(x.shape[0], c)
        want = (g_t * torch.from_numpy(scale.astype(np.float64)) + torch.from_numpy(shift.astype(np.float64))).numpy()
    g, emb, gbound, ebound = ref.gem(x, p, scale, shift)
    assert np.abs(g - g_t.numpy()).max() < 1e-12 and np.abs(emb - want).max() < 1e-12
    assert (ebound > 0).all() and ebound.max() < 1e-4
    with np.errstate(invalid="ignore"):
        _, wrong, _, _ = ref.gem(x, p, scale, shift, clamp=False)
    assert (~(np.abs(wrong - emb) <= 10 * ebound)).any(), "GeM without the clamp would pass"


# ---------------------------------------------------------------------------------------------- 2. sizes and passes
def test_pass_size_rule():
    """chunk * 256 * 128 / (h * w) clamped to 1 .. 4096: a pass never holds more input pixels than `chunk` crops of 256 x 128, so no
    stage of it is larger than that pass's (every stage scales with h * w up to the rounding of odd sides, which the floor covers)."""
    assert engine_mod.any_pass_size(1024, 256, 128) == 1024 == ref.pass_size(1024, 256, 128)
    assert engine_mod.any_pass_size(1024, 224, 268) == 1024 * 32768 // (224 * 268) == 558
    assert engine_mod.any_pass_size(1024, 64, 32) == 4096 and engine_mod.any_pass_size(1, 512, 512) == 1
    assert engine_mod.any_pass_size(5, 96, 72) == 23
    for chunk in (1, 7, 64, 1024, 4096):
        for h, w in ((32, 32), (64, 32), (96, 72), (224, 251), (224, 268), (511, 509), (512, 512)):
            p = engine_mod.any_pass_size(chunk, h, w)
            assert p == ref.pass_size(chunk, h, w) and 1 <= p <= 4096
            assert p == 1 or p == 4096 or p * h * w <= chunk * 32768 < (p + 1) * h * w
    assert engine_mod.stage_shapes(256, 128) == ref.stage_shapes(256, 128)
    assert [a * b * c for a, b, c in ref.stage_shapes(256, 128)] == [524288, 131072, 131072, 131072, 65536, 65536, 32768, 32768, 65536, 65536]
    assert ref.stage_shapes(96, 72)[2:] == [(24, 18, 64)] * 2 + [(12, 9, 128)] * 2 + [(6, 5, 256)] * 2 + [(6, 5, 512)] * 2
    assert ref.stage_shapes(224, 268)[2][:2] == (56, 67) and ref.stage_shapes(224, 268)[-1][:2] == (14, 17)
    assert ref.stage_shapes(64, 32)[-1] == (4, 2, 512) and engine_mod.stage_shapes(97, 75) == ref.stage_shapes(97, 75)


class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    PIL_MAX_SIDE = Engine.PIL_MAX_SIDE
    _swin_crop_args = staticmethod(Engine._swin_crop_args)
    _pack_ragged = staticmethod(Engine._pack_ragged)
    _pack_images = classmethod(Engine._pack_images.__func__)

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


@pytest.mark.parametrize("size", [(31, 128), (256, 513), (0, 0), (224,), (224.5, 268), "veri", (224, 268, 3)])
def test_a_bad_size_raises_before_any_device_call(size):
    eng = _NoDevice()
    crops = [np.zeros((9, 7, 3), np.uint8)]
    with pytest.raises(ValueError):
        engine_mod.check_hw(size)
    with pytest.raises(ValueError):
        Engine.embed_ragged_u8(eng, crops, size=size)
    with pytest.raises(ValueError):
        Engine.descriptor_images_u8(eng, crops, size=size)
    with pytest.raises(ValueError):
        Engine.descriptor_dev(eng, 1, 1, True, 1, size=size)
    with pytest.raises(ValueError):
        Engine.embed_f32_nchw_dev(eng, 1, 1, 1, size=size)
    with pytest.raises(ValueError):
        inference_utils.extract_descriptors(crops, size=size)
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=size)
    lab = np.zeros(1, np.int64)
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="seres18_hw", size=size)


def test_python_size_rules():
    eng = _NoDevice()
    assert engine_mod.check_hw((224, 268)) == (224, 268) and engine_mod.check_hw(np.asarray([32, 512])) == (32, 512)
    for shape in ((2, 3, 31, 128), (2, 3, 256, 600), (2, 4, 256, 128), (3, 256, 128)):
        with pytest.raises(ValueError):
            Engine.embed_f32_nchw(eng, np.zeros(shape, np.float32))
        with pytest.raises(ValueError):
            Engine.descriptor_f32_nchw(eng, np.zeros(shape, np.float32))
        with pytest.raises(ValueError):
            seres18_ibn(num_classes=5)(np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="seres18_ibn"):
        cares18_ibn(num_classes=5)(np.zeros((1, 3, 96, 72), np.float32))           # the siblings stay at 256 x 128
    with pytest.raises(ValueError, match="size"):
        reid_inference.inference_efficient(eng, [np.zeros((9, 7, 3), np.uint8)], 1, arch="seres18_hw")      # uint8 images need their target
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 20, 20), np.float32), 1, arch="seres18_hw")
    with pytest.raises(ValueError, match="256"):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 224, 268), np.float32), 1)                  # "seres18" stays fixed
    with pytest.raises(ValueError, match="size"):
        inference_utils.extract_descriptors(np.zeros((1, 3, 96, 72), np.float32), size=(224, 268))
    assert "seres18_hw" in reid_inference.ARCHS
    # the extractor: another size is exact fp32 and has to be asked for as such; the siblings have no other size
    sd = synth.seres18_state_dict(0)
    with pytest.raises(ValueError, match="f32"):
        Extractor(sd, size=(64, 128))
    with pytest.raises(ValueError):
        Extractor(sd, size=(64, 1000), precision="f32")


# ---------------------------------------------------------------------------------------------- 3. the side library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """The kernels live in a library of their own that libreid_hip.so opens from its own directory on the first call at another size: its
    kernel list equals tests/golden/kernels_anysize.json by name, no kernel has scratch or AGPRs or more VGPRs than the list allows, the
    product library does not name the file among what it needs, and it loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 6
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values()), {k: v["vgprs"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    lib = ctypes.CDLL(LIB)
    for sym in SIDE_SYMBOLS:
        assert hasattr(lib, sym)


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    for sym in ENTRIES:
        assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym), sym
    dbg = _ffi.debug_lib()
    for sym in HARNESSES:
        assert sym + "(" in dbg_hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(dbg, sym), sym
    assert "anysize_force" in dbg_hdr
    for name in ("debug_any_norm", "debug_any_se_tail", "debug_any_gem"):
        assert callable(getattr(Engine, name))


def test_fixture_holds_the_three_cases(golden_dir):
    """tests/golden/anysize.npz: seeds, sizes, the eleven taps, embeddings, logits and descriptors of the three cases - nothing else,
    nothing large."""
    path = os.path.join(golden_dir, "anysize.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    assert int(z["n_cases"]) == 3 and int(z["weight_seed"]) == 0
    names = ["bn0", "pooling0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["avgpooling"]
    want = [(64, 32, 3), (96, 72, 3), (224, 268, 2)]
    for k, (h, w, n) in enumerate(want):
        p = "c%d_" % k
        assert (int(z[p + "h"]), int(z[p + "w"]), int(z[p + "n"])) == (h, w, n)
        assert z[p + "emb"].shape == (n, 512) and z[p + "logits"].shape == (n, 751)
        assert z[p + "desc_tta"].shape == z[p + "desc_plain"].shape == (n, 1263)
        np.testing.assert_allclose(np.linalg.norm(z[p + "desc_tta"], axis=1), 1.0, atol=1e-5)
        shapes = ref.stage_shapes(h, w)
        for s, name in enumerate(names[:10]):
            assert tuple(z[p + "shape_" + name]) == (n, shapes[s][2], shapes[s][0], shapes[s][1]), (k, name)
            assert z[p + "tap_" + name].size <= 3 * 8 * 16 * 8
        assert len([f for f in z.files if f.startswith(p + "tap_")]) == 11
