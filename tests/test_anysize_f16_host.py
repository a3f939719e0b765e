"""Host side of the fp16-storage any-size forward (no GPU): the side library's kernel list and independence, the declared / bound /
exported surface, the fp16-storage restatement of the forward (tests/anysize_f16_ref.py) against the reference fixture, one mutation per
kernel family that the GPU checks of tests/test_gpu_anysize_f16.py would catch - shown on the numpy oracles with that module's own cases
and bounds -, and the Python rules of the hw_f16 keyword up to the first device call."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import seres18
from reid_amd import _ffi, inference_utils, reid_inference, synth
from reid_amd.backbone import cares18_ibn, emares18_ibn, seres18_ibn
from reid_amd.engine import Engine
from reid_amd.extractor import Extractor
from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_f16_ref as r  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize_f16.so")
SIDE_EXPORTS = ("anysize_f16_conv", "anysize_f16_stem", "anysize_f16_maxpool", "anysize_f16_norm", "anysize_f16_se_tail", "anysize_f16_gem")
HARNESSES = ("reid_debug_any_conv_f16", "reid_debug_any_stem_f16", "reid_debug_any_norm_f16", "reid_debug_any_se_tail_f16",
             "reid_debug_any_gem_f16")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _kernel_rows(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(lib)
    names = sorted(rows)
    return {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}


# ---------------------------------------------------------------------------------------------- 1. the library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_f16.so holds the kernels of tests/golden/kernels_anysize_f16.json by name, none with scratch, none over the
    register or LDS cap that two blocks per CU allow; no kernel of it is in the product library, whose own list is what
    tests/golden/kernels.json says; the product library does not name the file among what it needs, the side library needs nothing of
    the project's, and it loads on its own, without a GPU."""
    got = _kernel_rows(LIB)
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_f16.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(0 < v["vgprs"] + v["agprs"] <= spec["max_regs"] for v in got.values()), {k: (v["vgprs"], v["agprs"]) for k, v in got.items()}
    assert all(v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    assert any("any_conv_f16_kernel<64>" in k for k in got) and any("any_conv_f16_kernel<128>" in k for k in got)
    product = _kernel_rows(_ffi.LIB_PATH)
    listed = json.load(open(os.path.join(golden_dir, "kernels.json")))["kernels"]
    assert sorted(product) == sorted(listed) and not set(product) & set(got)
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    side = ctypes.CDLL(LIB)
    assert all(hasattr(side, s) for s in SIDE_EXPORTS)


def test_the_setting_and_the_harnesses_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    sym = "reid_ctx_set_hw_f16"
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(reid_[a-z0-9_]+)$", nm, re.M))
    assert sym in declared and sym in _ffi.EXPORTS and sym in exported
    assert _ffi._SIGS[sym] == _ffi._SIGS["reid_ctx_set_hw_ema"] and hasattr(ctypes.CDLL(_ffi.LIB_PATH), sym)
    nm_dbg = subprocess.run(["nm", "-D", "--defined-only", _ffi.DEBUG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in HARNESSES:
        assert re.search(r"^int %s\(" % name, dbg_hdr, re.M) and name in _ffi.DEBUG_EXPORTS and re.search(r"\sT\s+%s$" % name, nm_dbg, re.M), name
    for name in ("hw_f16_value", "set_hw_f16", "hw_f16", "hw_f16_scope", "debug_any_conv_f16", "debug_any_stem_f16", "debug_any_norm_f16",
                 "debug_any_se_tail_f16", "debug_any_gem_f16"):
        assert hasattr(Engine, name), name
    assert "has no any-size forward" not in Engine.hw_precision_value.__doc__
    mk = open(os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc", "Makefile")).read()
    assert "ANYF16_OUT = ../libreid_hip_anysize_f16.so" in mk and "$(ANYF16_OUT)" in mk.split("all:")[1].split("\n")[0]


# ---------------------------------------------------------------------------------------------- 2. the restated forward
@pytest.mark.parametrize("k", r.FORWARD_CASES)
def test_restated_forward_meets_the_mode_1_limits(golden_dir, k):
    """The arithmetic alone (f16 input, weights and stored activations, everything else float64) against the reference's own class:
    1 - cos < 1e-4 and 2e-2 of the largest magnitude, the limits the GPU test applies to the kernels."""
    fx = np.load(os.path.join(golden_dir, "anysize.npz"))
    p = "c%d_" % k
    h, w, n, seed = (int(fx[p + key]) for key in ("h", "w", "n", "seed"))
    x = seres18.preprocess_u8(synth.smooth_crops_u8(n, seed, h, w))
    taps = {}
    emb, logits = r.forward_f16(synth.seres18_state_dict(0), x.numpy(), taps)
    we, wl = fx[p + "emb"].astype(np.float64), fx[p + "logits"].astype(np.float64)
    cos = 1.0 - (emb * we).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(we, axis=1)
    ee, le = np.abs(emb - we).max() / np.abs(we).max(), np.abs(logits - wl).max() / np.abs(wl).max()
    print("(%d, %d): 1 - cos %.3g, emb %.3g, logits %.3g of the largest magnitude" % (h, w, cos.max(), ee, le))
    assert cos.max() < r.COS_LIMIT and ee < r.EMB_LIMIT and le < r.EMB_LIMIT
    ref_taps = {}
    seres18.forward(synth.seres18_state_dict(0), x, ref_taps)
    for name in ["stem", "pool0"] + [b[0] for b in seres18.BLOCKS] + ["gem"]:
        want = ref_taps[name].numpy().astype(np.float64)
        err = np.abs(taps[name].numpy() - want).max() / np.abs(want).max()
        print("  %s: %.3g" % (name, err))
        assert err < r.STAGE_LIMIT, name


# ---------------------------------------------------------------------------------------------- 3. one mutation per kernel family
@pytest.mark.parametrize("name", ("l1", "l2s", "l4"))
def test_mutation_a_padding_tap_read_as_a_pixel(name):
    """Padding taps that read the nearest pixel instead of zero: outside the bound of the random case, other bits on the exact family."""
    cin, cout, rr, stride, h, w, n = r.GEOMS[name]
    kw, x, wt, want, bound = r.conv_case(name, 21)
    acc_m, _ = r.conv_oracle(x, wt, stride, pad_mode="edge")
    wrong = r.epilogue(acc_m, kw["scale"], kw["shift"], kw.get("res"), kw.get("relu", False), kw.get("relu_from", 0))
    over = float((np.abs(wrong - want) > bound).mean())
    print("%s: %.0f %% of the outputs leave the bound" % (name, 100 * over))
    assert over > 0.2
    xe, we = r.exact_operands(name, 11)
    a, ab = r.conv_oracle(xe, we, stride)
    assert ab.max() < 2.0 ** 24 and np.array_equal(a, np.round(a))
    am, _ = r.conv_oracle(xe, we, stride, pad_mode="edge")
    assert (a.astype(np.float16).view(np.uint16) != am.astype(np.float16).view(np.uint16)).mean() > 0.2


@pytest.mark.parametrize("name", ("l1", "l1big"))
def test_mutation_the_ragged_tiles_last_row_dropped(name):
    """M = 105 and 506 are no multiples of the 128-row tile.  A kernel that drops the last row leaves it unwritten (NaN from the harness:
    refused outright) or zero: outside the bound on that row, other bits on the exact family."""
    cin, cout, rr, stride, h, w, n = r.GEOMS[name]
    kw, x, wt, want, bound = r.conv_case(name, 21)
    assert want.shape[0] % 128 != 0
    wrong = want.copy()
    wrong[-1] = 0.0
    over = np.abs(wrong - want) > bound                                    # with ReLU on, the outputs that are 0 anyway stay inside
    print("%s: %.0f %% of the last row leaves the bound" % (name, 100 * over[-1].mean()))
    assert over[-1].mean() > 0.2 and not over[:-1].any()
    xe, we = r.exact_operands(name, 11)
    a, _ = r.conv_oracle(xe, we, stride)
    assert (a[-1].astype(np.float16) != 0).any()


@pytest.mark.parametrize("c", r.TAIL_CS)
@pytest.mark.parametrize("hw", r.TAIL_HWS)
def test_mutation_unbiased_variance(hw, c):
    x, half, gamma, beta = r.norm_case(hw, c)
    want, bound = r.norm_oracle(x, gamma, beta, half)
    wrong, _ = r.norm_oracle(x, gamma, beta, half, sample_variance=True)
    over = float((np.abs(wrong - want) > bound).mean())
    print("hw %d c %d: %.0f %% of the outputs leave the bound" % (hw, c, 100 * over))
    assert over > 0.2


@pytest.mark.parametrize("c", r.TAIL_CS)
@pytest.mark.parametrize("hw", r.TAIL_HWS)
def test_mutation_the_gate_applied_before_the_residual(hw, c):
    y, sc, w1, w2t = r.se_case(hw, c)
    want, gate, bound, gbound = r.se_oracle(y, sc, w1, w2t)
    wrong = r.se_oracle(y, sc, w1, w2t, gate_first=True)[0]
    over = float((np.abs(wrong - want) > bound).mean())
    print("hw %d c %d: %.0f %% of the outputs leave the bound" % (hw, c, 100 * over))
    assert over > 0.2
    assert (np.abs(r.f16(want) - want) <= bound).all()               # the faithful value, rounded once, is inside


@pytest.mark.parametrize("size", r.STEM_SIZES, ids=["%dx%d" % s for s in r.STEM_SIZES])
def test_mutation_a_zero_padded_max_pool(size):
    """MaxPool2d pads with -inf; the stem has no ReLU, so border windows whose pixels are all negative tell a 0-padded pool apart."""
    x, wt, scale, shift = r.stem_operands(size[0], size[1], 41)
    want, bound = r.stem_oracle(x, wt, scale, shift)
    stem = r.f16(want)
    assert (np.abs(stem - want) <= bound).all()
    good, wrong = r.maxpool(stem), r.maxpool(stem, 0.0)
    h1, w1 = (size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1
    assert good.shape == (r.STEM_N, (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1, 64) and np.isfinite(good).all()
    differs = good != wrong
    assert differs.any() and not differs[:, 1:-1, 1:-1].any()              # only windows that reach over the border can differ
    assert (wrong[differs] == 0.0).all()


def test_the_stem_weights_are_the_f16_image_of_the_packed_rows():
    """The forward hands the kernel the f16 copy of weights.stem_pack's [64][8][24] rows: stem_pack16 builds exactly those."""
    from reid_amd import weights
    w = np.random.default_rng(3).normal(size=(64, 3, 7, 7)).astype(np.float32)         # torch layout [cout, c, r, s]
    packed = np.asarray(weights.stem_pack(w), np.float32).reshape(64, 192)
    assert np.array_equal(packed.astype(np.float16), r.stem_pack16(w.transpose(0, 2, 3, 1)))


# ---------------------------------------------------------------------------------------------- 4. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    hw_precision_value = staticmethod(Engine.hw_precision_value)
    hw_f16_value = staticmethod(Engine.hw_f16_value)

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_hw_f16_values_and_the_scope():
    eng = _NoDevice()
    for v, want in ((False, 0), (True, 1), (0, 0), (1, 1), (np.int32(1), 1), (np.bool_(True), 1)):
        assert Engine.hw_f16_value(v) == want
    for bad in (2, -1, "f16", None, 1.0, (1,)):
        with pytest.raises(ValueError, match="hw_f16"):
            Engine.hw_f16_value(bad)
        with pytest.raises(ValueError):
            Engine.set_hw_f16(eng, bad)                                    # before the C ABI is reached

    class _Rec:
        hw_f16 = False
        calls = []

        def set_hw_f16(self, on):
            self.calls.append(on)
            self.hw_f16 = bool(on)
    rec = _Rec()
    with Engine.hw_f16_scope(rec, None):
        assert rec.calls == []
    with pytest.raises(KeyError):
        with Engine.hw_f16_scope(rec, True):
            assert rec.hw_f16 is True
            raise KeyError("x")
    assert rec.hw_f16 is False and rec.calls == [True, False]               # restored after a failing call too
    rec.hw_f16 = True
    with Engine.hw_f16_scope(rec, True):
        pass
    assert rec.hw_f16 is True                                              # what it was before


def test_inference_rules():
    eng = _NoDevice()
    crops = [np.zeros((9, 7, 3), np.uint8)]
    lab = np.zeros(1, np.int64)
    with pytest.raises(ValueError, match="hw_f16.*hw_precision"):
        inference_utils.extract_descriptors(crops, size=(96, 72), hw_f16=True, hw_precision="f32")
    with pytest.raises(ValueError, match="hw_f16"):
        inference_utils.extract_descriptors(crops, size=(96, 72), hw_f16="on")
    for arch in ("seres18", "cares18_hw", "swin"):
        with pytest.raises(ValueError, match="hw_f16.*seres18_hw"):
            reid_inference.inference_efficient(eng, crops, 1, arch=arch, hw_f16=True)
        with pytest.raises(ValueError, match="hw_f16.*seres18_hw"):
            reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch=arch, hw_f16=True)
    with pytest.raises(ValueError, match="hw_f16.*seres18_hw"):
        reid_inference.inference_efficient(eng, crops, 1, arch="emares18_hw", hw_ema=True, hw_f16=True)
    with pytest.raises(ValueError, match="hw_f16.*hw_precision"):
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=(96, 72), hw_f16=True, hw_precision="f16x3")
    with pytest.raises(ValueError, match="hw_f16.*hw_precision"):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="seres18_hw", size=(96, 72), hw_f16=True,
                                     hw_precision="f32")
    with pytest.raises(ValueError, match="hw_f16"):
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=(96, 72), hw_f16=2)
    with pytest.raises(ValueError):                                        # a bad size still raises, before the engine
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=(31, 72), hw_f16=True)


def test_extractor_and_model_rules(monkeypatch):
    sd = synth.seres18_state_dict(0)

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    monkeypatch.delenv("REID_PRECISION", raising=False)
    for kw in ({}, {"precision": "f16"}, {"precision": "f32"}):
        with pytest.raises(_Stop):                                         # the keyword names the arithmetic: the next step is the engine
            Extractor(sd, size=(64, 128), hw_f16=True, **kw)
    with pytest.raises(ValueError, match="f32"):                           # without it the existing rule holds
        Extractor(sd, size=(64, 128))
    with pytest.raises(ValueError, match="hw_f16"):
        Extractor(sd, size=(64, 128), hw_f16="yes")
    for make, kw in ((synth.cares18_state_dict, {"hw_siblings": True}), (synth.emares18_state_dict, {"hw_ema": True})):
        with pytest.raises(ValueError, match="hw_f16.*seres18_ibn"):
            Extractor(make(0), size=(64, 128), precision="f32", hw_f16=True, **kw)
    with pytest.raises(ValueError):
        Extractor(sd, size=(31, 128), hw_f16=True)
    assert seres18_ibn(num_classes=5)._hw_f16 is False and seres18_ibn(num_classes=5, hw_f16=True)._hw_f16 is True
    for factory in (cares18_ibn, emares18_ibn):
        with pytest.raises(ValueError, match="hw_f16"):
            factory(num_classes=5, hw_f16=True)
    with pytest.raises(ValueError, match="hw_f16.*hw_precision"):
        seres18_ibn(num_classes=5, hw_f16=True, hw_precision="f16x3")
    with pytest.raises(ValueError, match="hw_f16"):
        seres18_ibn(num_classes=5, hw_f16=3)
    with pytest.raises(ValueError):                                        # a bad size is refused before the engine
        seres18_ibn(num_classes=5, hw_f16=True)(np.zeros((1, 3, 31, 72), np.float32))
    from reid_amd.models import build_model
    assert build_model("seres18_ibn", 5, loss="triplet", pretrained=False, hw_f16=True)._hw_f16 is True
    for name in ("cares18_ibn", "emares18_ibn", "swin_transformer"):
        with pytest.raises(ValueError, match="hw_f16"):
            build_model(name, 5, pretrained=False, hw_f16=True)


def test_stream_rules():
    blob = np.zeros(4, np.float32)
    for cls, extra in ((CameraStream, ()), (MultiCameraStream, (2,)), (LookaheadCameraStream, ())):
        for arch in ("seres18", "swin", "cares18_hw"):
            with pytest.raises(ValueError, match="hw_f16"):
                cls(blob, "", *extra, arch=arch, hw_f16=True)
        with pytest.raises(ValueError, match="hw_f16"):
            cls(blob, "", *extra, arch="emares18_hw", hw_ema=True, size=(128, 64), hw_f16=True)
        with pytest.raises(ValueError, match="hw_f16.*hw_precision"):
            cls(blob, "", *extra, arch="seres18_hw", size=(128, 64), hw_f16=True, hw_precision="f16x3")
        with pytest.raises(ValueError, match="hw_f16"):
            cls(blob, "", *extra, arch="seres18_hw", size=(128, 64), hw_f16="x")
        with pytest.raises(ValueError):
            cls(blob, "", *extra, arch="seres18_hw", size=(31, 64), hw_f16=True)
