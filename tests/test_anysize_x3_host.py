"""Host side of the fp32-class any-size forward (no GPU): the side library's kernel list and independence, the declared / bound / exported
surface, the numpy restatement of the split arithmetic on the two input families the GPU tests rely on (tests/anysize_x3_ref.py) with
the mutations those families are there to catch, and the Python rules up to the first device call."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, inference_utils, reid_inference, synth
from reid_amd.backbone import cares18_ibn, seres18_ibn
from reid_amd.engine import Engine
from reid_amd.extractor import Extractor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_x3_ref as x3  # noqa: E402
from test_gpu_conv import bound, conv_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize_x3.so")
K_CASES = ("l2d", "l1", "l4")        # K = 64, 576, 4608


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


# ---------------------------------------------------------------------------------------------- 1. the library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_x3.so holds the kernels of tests/golden/kernels_anysize_x3.json by name, none with scratch or AGPRs, none over
    the VGPR or LDS cap that two blocks per CU allow; the product library does not name the file among what it needs, the side library
    needs nothing of the project's, and it loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_x3.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values()), {k: v["vgprs"] for k, v in got.items()}
    assert all(0 < v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    assert hasattr(ctypes.CDLL(LIB), "anysize_x3_conv")


def test_the_setting_and_the_harness_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    sym = "reid_ctx_set_hw_precision"
    assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    assert "reid_debug_any_conv(" in dbg_hdr and "reid_debug_any_conv" in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), "reid_debug_any_conv")
    for name in ("set_hw_precision", "hw_precision", "hw_precision_scope", "debug_any_conv"):
        assert hasattr(Engine, name), name


# ---------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("name", sorted(x3.GEOMS))
def test_exact_family_is_exact_in_fp32(name):
    """Every term is a multiple of 0.25 and sum |terms| / 0.25 < 2^24: fp32 accumulation is exact in any order, the three-product value is
    one fp32 number.  numpy's split gives xh in {0, +-1} and xl' in {0, +-0.25}.  Dropping either cross product changes most outputs."""
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    x, wt = x3.exact_operands(name, 11)
    xh, xl = x3.split(x)
    wh, wl = x3.split(wt)
    assert set(np.unique(xh)) <= {-1.0, 0.0, 1.0} and set(np.unique(xl)) <= {-0.25, 0.0, 0.25}
    assert set(np.unique(wh)) == {-1.0, 1.0} and set(np.unique(wl)) <= {-0.25, 0.0, 0.25}
    val, mag = x3.restate(x, wt, stride)
    quarters = mag.max() / 0.25
    print("%s: K %d, largest sum |terms| / 0.25 = %.3g" % (name, r * r * cin, quarters))
    assert quarters < 2.0 ** 24
    assert np.array_equal(val * 2048.0 * 4.0, np.round(val * 2048.0 * 4.0))
    assert np.array_equal(val.astype(np.float32).astype(np.float64), val)            # one fp32 number
    for drop in ("lh", "hl"):
        wrong, _ = x3.restate(x, wt, stride, drop=drop)
        changed = float((wrong != val).mean())
        print("%s: without the %s product %.0f %% of the outputs change" % (name, drop, 100 * changed))
        assert changed > 0.5


@pytest.mark.parametrize("name", K_CASES)
def test_small_family_needs_f16_subnormals(name):
    """x ~ N(0, 1) 2^-15: the faithful restatement stays far below bound(..., split=True); with f16 subnormals flushed in both parts it is
    orders of magnitude over it, and with xl' alone flushed it is over it at K = 64 and 576."""
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    k = r * r * cin
    x, wt = x3.small_operands(name, 12)
    ho, wo = x3.out_hw(name)
    acc, ab = conv_oracle(x, wt, stride, x3.pad_of(r), np.arange(n * ho * wo))
    b = bound(acc, ab, wt, k, True)
    val, _ = x3.restate(x, wt, stride)
    good = float((np.abs(val - acc) / b).max())
    both = float((np.abs(x3.restate(x, wt, stride, flush_hi=True, flush_lo=True)[0] - acc) / b).max())
    lo = float((np.abs(x3.restate(x, wt, stride, flush_lo=True)[0] - acc) / b).max())
    print("%s (K %d): err / bound faithful %.3g, both parts flushed %.3g, xl' flushed %.3g" % (name, k, good, both, lo))
    assert good < 0.1
    assert both > 10.0
    if k <= 576:
        assert lo > 1.0


@pytest.mark.parametrize("name", ("l1", "l4"))
def test_the_float64_bound_alone_misses_a_dropped_product(name):
    """Why the exact family exists: on random operands a dropped xl'.wh stays inside the float64 bound at K = 576 and 4608."""
    cin, cout, r, stride, h, w, n = x3.GEOMS[name]
    x, wt = x3.random_operands(name, 13)[:2]
    ho, wo = x3.out_hw(name)
    acc, ab = conv_oracle(x, wt, stride, x3.pad_of(r), np.arange(n * ho * wo))
    b = bound(acc, ab, wt, r * r * cin, True)
    wrong, _ = x3.restate(x, wt, stride, drop="lh")
    assert (np.abs(wrong - acc) <= b).all()


# ---------------------------------------------------------------------------------------------- 3. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    hw_precision_value = staticmethod(Engine.hw_precision_value)

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_hw_precision_values():
    eng = _NoDevice()
    for v, want in ((None, -1), (-1, -1), (0, 0), (2, 2), ("f32", 0), ("f16x3", 2), (" F16x3 ", 2), (np.int32(2), 2)):
        assert Engine.hw_precision_value(v) == want
    for bad in (1, 3, -2, "f16", "", 2.0, True, (2,)):
        with pytest.raises(ValueError):
            Engine.hw_precision_value(bad)
        with pytest.raises(ValueError):
            Engine.set_hw_precision(eng, bad)                              # before the C ABI is reached
    crops = [np.zeros((9, 7, 3), np.uint8)]
    with pytest.raises(ValueError):
        inference_utils.extract_descriptors(crops, size=(96, 72), hw_precision="f16")
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=(96, 72), hw_precision=1)
    with pytest.raises(ValueError, match="seres18_hw"):
        reid_inference.inference_efficient(eng, np.zeros((1, 3, 256, 128), np.float32), 1, hw_precision="f16x3")
    lab = np.zeros(1, np.int64)
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="seres18_hw", size=(96, 72),
                                     hw_precision="f16")
    with pytest.raises(ValueError):                                        # a bad size still comes first
        reid_inference.inference_efficient(eng, crops, 1, arch="seres18_hw", size=(31, 72), hw_precision="f16x3")


def test_extractor_and_model_rules(monkeypatch):
    sd = synth.seres18_state_dict(0)

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    with pytest.raises(_Stop):                                             # the argument checks pass: the next step is the engine
        Extractor(sd, size=(64, 128), precision="f16x3")
    with pytest.raises(ValueError):
        Extractor(sd, size=(64, 128), precision="f16")
    with pytest.raises(ValueError, match="f32"):
        Extractor(sd, size=(64, 128))
    monkeypatch.setenv("REID_PRECISION", "f16x3")                          # a default, not "asked by name"
    with pytest.raises(ValueError, match="f32"):
        Extractor(sd, size=(64, 128))
    monkeypatch.delenv("REID_PRECISION")
    with pytest.raises(ValueError):
        Extractor(synth.cares18_state_dict(0), size=(64, 128), precision="f16x3")
    with pytest.raises(ValueError, match="seres18_ibn"):
        cares18_ibn(num_classes=5, hw_precision="f16x3")(np.zeros((1, 3, 96, 72), np.float32))
    with pytest.raises(ValueError):
        seres18_ibn(num_classes=5, hw_precision="f16")
    with pytest.raises(ValueError):
        seres18_ibn(num_classes=5, hw_precision="f16x3")(np.zeros((1, 3, 31, 72), np.float32))
    assert seres18_ibn(num_classes=5)._hw_call is None and seres18_ibn(num_classes=5, hw_precision="f16x3")._hw_call is not None
    from reid_amd.models import build_model
    assert build_model("seres18_ibn", 5, loss="triplet", pretrained=False, hw_precision="f16x3")._hw_call is not None
    with pytest.raises(ValueError):
        build_model("swin_transformer", 5, pretrained=False, hw_precision="f16x3")
