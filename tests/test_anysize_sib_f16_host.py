"""Host side of CARes18-IBN / EMARes18-IBN at any input size in fp16 storage (no GPU): the operand families stay inside f16's range, the
fp16-storage restatement of both forwards (tests/anysize_sib_f16_ref.py) meets the forward limits on the reference fixtures, one mutation per
tail that the GPU checks of tests/test_gpu_anysize_sib_f16.py would catch - shown on the numpy oracles with that module's own cases and
bounds -, the side library's kernel list, independence, exports and workspace queries, the declared / bound / exported surface, and the
Python rules of the hw_sib_f16 keyword up to the first device call."""
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
from reid_amd.backbone import cares18_ibn, emares18_ibn, seres18_ibn, swin_t
from reid_amd.engine import Engine
from reid_amd.extractor import Extractor
from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import so_kernels  # noqa: E402
import anysize_ca_ref as ca  # noqa: E402
import anysize_ema_ref as ema  # noqa: E402
import anysize_f16_ref as f16r  # noqa: E402
import anysize_sib_f16_ref as r  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-reid-tracking_amd")
LIB = os.path.join(PKG, "libreid_hip_anysize_sib_f16.so")
SIDE_EXPORTS = ("anysize_sib_f16_ca_tail", "anysize_sib_f16_ca_workspace_bytes", "anysize_sib_f16_ema_tail", "anysize_sib_f16_ema_workspace_bytes")
HARNESSES = ("reid_debug_any_ca_tail_f16", "reid_debug_any_ema_tail_f16")
MAKE_SD = {"cares18_ibn": synth.cares18_state_dict, "emares18_ibn": synth.emares18_state_dict}
CA_MUTATIONS = ("biased", "swap_channels", "swap_cw_hc", "transposed_plane", "replicate", "third_on_two", "shortcut_first")
CA_SMALL, EMA_SMALL = r.CA_CASES[:4], r.EMA_CASES[:7]                      # the mutations need no large map


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


# ---------------------------------------------------------------------------------------------- 1. operands
@pytest.mark.parametrize("kind", ["ca", "ema"])
def test_operand_families_stay_inside_f16s_range(kind):
    """Every family of both tails, every case, rounded to float16: finite, and what the rounding did to a value is at most half an ulp."""
    cases, fams, ops = (r.CA_CASES, r.CA_FAMILIES, ca.operands) if kind == "ca" else (r.EMA_CASES, r.EMA_FAMILIES, ema.operands)
    for case in cases:
        for family in fams:
            n = r.batches(case)[-1]
            y, sc = ops(case, n, family)
            for a in (y, sc):
                a16 = a.astype(np.float16)
                assert np.isfinite(a16).all() and np.abs(a).max() < r.F16_MAX, (case, family)
                assert (np.abs(a16.astype(np.float64) - a) <= f16r.H * np.abs(a) + f16r.H_ABS).all(), (case, family)
    y16, sc16, prm = (r.ca_operands if kind == "ca" else r.ema_operands)(cases[0], 3, fams[0])
    assert y16.dtype == sc16.dtype == np.float16 and prm.dtype == np.float32


# ---------------------------------------------------------------------------------------------- 2. the restated forwards
@pytest.mark.parametrize("k", r.FORWARD_CASES)
@pytest.mark.parametrize("arch", sorted(r.ARCHS))
def test_restated_forward_meets_the_mode_1_limits(golden_dir, arch, k):
    """The arithmetic alone (f16 input, weights and stored activations, everything else float64) against the reference's own class on
    tests/golden/anysize_ca.npz / anysize_ema.npz: 1 - cos < 1e-4, embeddings, logits and block taps within 2e-2 of the largest magnitude -
    the limits the GPU test applies to the kernels are reachable."""
    fx = np.load(os.path.join(golden_dir, r.ARCHS[arch]))
    p = "c%d_" % k
    h, w, n, seed = (int(fx[p + key]) for key in ("h", "w", "n", "seed"))
    x = seres18.preprocess_u8(synth.smooth_crops_u8(n, seed, h, w))
    taps = {}
    emb, logits = r.forward_sib_f16(MAKE_SD[arch](int(fx["weight_seed"])), x.numpy(), arch, taps)
    we, wl = fx[p + "emb"].astype(np.float64), fx[p + "logits"].astype(np.float64)
    cos = 1.0 - (emb * we).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(we, axis=1)
    ee, le = np.abs(emb - we).max() / np.abs(we).max(), np.abs(logits - wl).max() / np.abs(wl).max()
    print("%s (%d, %d): 1 - cos %.3g, emb %.3g, logits %.3g of the largest magnitude" % (arch, h, w, cos.max(), ee, le))
    assert cos.max() < r.COS_LIMIT and ee < r.EMB_LIMIT and le < r.EMB_LIMIT
    for name in [b[0] for b in seres18.BLOCKS]:
        want = fx[p + "tap_" + name].astype(np.float64)
        got = r.sample_nchw(taps[name].numpy())
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got - want).max() / np.abs(want).max()
        print("  %s: %.3g" % (name, err))
        assert err < r.STAGE_LIMIT, name
        assert np.array_equal(got, f16r.f16(got)), name                    # a stored tap is an f16 value


# ---------------------------------------------------------------------------------------------- 3. mutations the GPU bound would catch
@pytest.fixture(scope="module")
def ca_table():
    return [(case, fam, r.ca_case(case, r.batches(case)[-1], fam)) for case in CA_SMALL for fam in r.CA_FAMILIES]


@pytest.fixture(scope="module")
def ema_table():
    return [(case, fam, r.ema_case(case, r.batches(case)[-1], fam)) for case in EMA_SMALL for fam in r.EMA_FAMILIES]


def test_the_oracles_own_rounding_stays_inside_the_store_bound(ca_table, ema_table):
    """float16(oracle output) is what a perfect tail stores: inside store_bound everywhere (so the bound admits the correct answer)."""
    for case, fam, d in ca_table:
        assert (np.abs(f16r.f16(d["out"]) - d["out"]) <= d["b_out"]).all(), (case, fam)
    for case, fam, d in ema_table:
        assert (np.abs(f16r.f16(d["want"]["out"]) - d["want"]["out"]) <= d["b_out"]).all(), (case, fam)


def test_mutation_statistics_through_f16_break_b32(ca_table, ema_table):
    """A tail that keeps its statistics in f16 - and so stores an output rounded twice - returns statistics outside b32: the ZPool maps
    and the gates of the TripletAttention tail, the sigmoid vectors, mu and rstd of the EMA tail, on every case and family."""
    for case, fam, d in ca_table:
        for name in ("maps", "gates"):
            assert (np.abs(r.twice_rounded(d[name]) - d[name]) > d["b_" + name]).any(), (case, fam, name)
    for case, fam, d in ema_table:
        broke = [name for name in ("sig", "mu", "rstd", "s2") if (np.abs(r.twice_rounded(d["want"][name]) - d["want"][name]) > d["b32"][name]).any()]
        assert "sig" in broke and "rstd" in broke, (case, fam, broke)


@pytest.mark.parametrize("mutation", CA_MUTATIONS)
def test_a_subtly_wrong_ca_tail_leaves_the_store_bound(ca_table, mutation):
    """The keyword mutations of tests/anysize_ca_ref.py, their output rounded to f16 as a kernel would store it."""
    caught = []
    for case, fam, d in ca_table:
        y, sc = d["y"].astype(np.float32), d["sc"].astype(np.float32)
        wrong = f16r.f16(ca.tail(y, sc, d["prm"], **{mutation: True})[0])
        if (np.abs(wrong - d["out"]) > d["b_out"]).any():
            caught.append((case, fam))
    print(mutation, "caught on", caught)
    assert caught, mutation + " would pass on every case"


@pytest.mark.parametrize("mutation", ema.MUTATIONS)
def test_a_subtly_wrong_ema_tail_leaves_the_store_bound(ema_table, mutation):
    """The MUTATIONS of tests/anysize_ema_ref.py, their output rounded to f16 as a kernel would store it."""
    caught = []
    for case, fam, d in ema_table:
        if mutation == "swap_pools" and case[0] == case[1]:
            continue
        y, sc = d["y"].astype(np.float32), d["sc"].astype(np.float32)
        wrong = f16r.f16(ema.tail(y, sc, d["prm"], **{mutation: True})["out"])
        if (np.abs(wrong - d["want"]["out"]) > d["b_out"]).any():
            caught.append((case, fam))
    print(mutation, "caught on", caught)
    assert caught, mutation + " would pass on every case"


# ---------------------------------------------------------------------------------------------- 4. the library and the surface
def _short(mangled, demangled):
    """name or name<args>, also where the demangler at hand does not know _Float16 (DF16_) and hands the symbol back."""
    if not demangled.startswith("_Z"):
        return so_kernels.short(demangled)
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    name, rest = mangled[m.end():][:int(m.group(1))], mangled[m.end():][int(m.group(1)):]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if not t:
        return name
    args = [v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([ib])(\d+)E", t.group(1))]
    return "%s<%s>" % (name, ", ".join(args))


def _kernel_rows(lib, shorten):
    rows = so_kernels.kernels(lib)
    names = sorted(rows)
    return {shorten(n, d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}


def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_sib_f16.so holds the kernels of tests/golden/kernels_anysize_sib_f16.json by name, none with scratch or AGPRs,
    none over the list's VGPRs or LDS (so none holds a slab of the map); no kernel of it is in the product library, whose own list is
    what tests/golden/kernels.json says; the product library does not name the file among what it needs, the side library needs nothing
    of the project's, and it loads on its own, without a GPU."""
    got = _kernel_rows(LIB, _short)
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_sib_f16.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(0 < v["vgprs"] <= spec["max_vgprs"] and v["agprs"] == 0 for v in got.values()), {k: (v["vgprs"], v["agprs"]) for k, v in got.items()}
    assert all(v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    product = _kernel_rows(_ffi.LIB_PATH, lambda n, d: so_kernels.short(d))
    listed = json.load(open(os.path.join(golden_dir, "kernels.json")))["kernels"]
    assert sorted(product) == sorted(listed) and not any("any_sib_" in k for k in product)
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own


def test_exports_and_workspace_queries(built):
    """The four exports; the workspace queries give the byte counts of the fp32 libraries for every case of both tables and both batch
    sizes, and 0 for a refused shape."""
    side = ctypes.CDLL(LIB)
    assert all(hasattr(side, s) for s in SIDE_EXPORTS)
    fp32 = {"ca": ctypes.CDLL(os.path.join(PKG, "libreid_hip_anysize_ca.so")).anysize_ca_workspace_bytes,
            "ema": ctypes.CDLL(os.path.join(PKG, "libreid_hip_anysize_ema.so")).anysize_ema_workspace_bytes}
    new = {"ca": side.anysize_sib_f16_ca_workspace_bytes, "ema": side.anysize_sib_f16_ema_workspace_bytes}
    for fn in list(fp32.values()) + list(new.values()):
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    for kind, cases in (("ca", r.CA_CASES), ("ema", r.EMA_CASES)):
        for h, w, c in cases + ((128, 128, 512), (2, 2, 64)):
            for n in (1, 3, 65535):
                assert new[kind](n, h, w, c) == fp32[kind](n, h, w, c) > 0, (kind, n, h, w, c)
        for n, h, w, c in ((1, 1, 4, 64), (1, 4, 129, 64), (1, 4, 4, 96), (0, 4, 4, 64), (65536, 4, 4, 64), (1, 4, 4, 1024)):
            assert new[kind](n, h, w, c) == 0, (kind, n, h, w, c)
    n, (h, w, c) = 3, r.CA_CASES[3]
    assert new["ca"](n, h, w, c) == n * 3 * (h * w + c * w + h * c) * 4


def test_the_setting_and_the_harnesses_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    sym = "reid_ctx_set_hw_sib_f16"
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(reid_[a-z0-9_]+)$", nm, re.M))
    assert sym in declared and sym in _ffi.EXPORTS and sym in exported
    assert _ffi._SIGS[sym] == _ffi._SIGS["reid_ctx_set_hw_f16"] and hasattr(ctypes.CDLL(_ffi.LIB_PATH), sym)
    nm_dbg = subprocess.run(["nm", "-D", "--defined-only", _ffi.DEBUG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in HARNESSES:
        assert re.search(r"^int %s\(" % name, dbg_hdr, re.M) and name in _ffi.DEBUG_EXPORTS and re.search(r"\sT\s+%s$" % name, nm_dbg, re.M), name
    for name in ("hw_sib_f16_value", "set_hw_sib_f16", "hw_sib_f16", "hw_sib_f16_scope", "debug_any_ca_tail_f16", "debug_any_ema_tail_f16"):
        assert hasattr(Engine, name), name
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "ANYSIBF16_OUT = ../libreid_hip_anysize_sib_f16.so" in mk and "$(ANYSIBF16_OUT)" in mk.split("all:")[1].split("\n")[0]
    assert "anysize_sib_f16.h" in [ln for ln in mk.split("\n") if ln.startswith("build/%.o:")][0]


# ---------------------------------------------------------------------------------------------- 5. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    hw_precision_value = staticmethod(Engine.hw_precision_value)
    hw_f16_value = staticmethod(Engine.hw_f16_value)
    hw_sib_f16_value = staticmethod(Engine.hw_sib_f16_value)

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_hw_sib_f16_values_and_the_scope():
    eng = _NoDevice()
    for v, want in ((False, 0), (True, 1), (0, 0), (1, 1), (np.int32(1), 1), (np.bool_(True), 1)):
        assert Engine.hw_sib_f16_value(v) == want
    for bad in (2, -1, "f16", None, 1.0, (1,)):
        with pytest.raises(ValueError, match="hw_sib_f16"):
            Engine.hw_sib_f16_value(bad)
        with pytest.raises(ValueError):
            Engine.set_hw_sib_f16(eng, bad)                                # before the C ABI is reached

    class _Rec:
        hw_sib_f16 = False
        calls = []

        def set_hw_sib_f16(self, on):
            self.calls.append(on)
            self.hw_sib_f16 = bool(on)
    rec = _Rec()
    with Engine.hw_sib_f16_scope(rec, None):
        assert rec.calls == []
    with pytest.raises(KeyError):
        with Engine.hw_sib_f16_scope(rec, True):
            assert rec.hw_sib_f16 is True
            raise KeyError("x")
    assert rec.hw_sib_f16 is False and rec.calls == [True, False]           # restored after a failing call too
    rec.hw_sib_f16 = True
    with Engine.hw_sib_f16_scope(rec, True):
        pass
    assert rec.hw_sib_f16 is True                                          # what it was before


def test_inference_rules():
    eng = _NoDevice()
    crops = [np.zeros((9, 7, 3), np.uint8)]
    lab = np.zeros(1, np.int64)
    for extra in ({"hw_precision": "f32"}, {"hw_f16": True}):
        with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision.*hw_f16"):
            inference_utils.extract_descriptors(crops, size=(96, 72), hw_sib_f16=True, **extra)
    with pytest.raises(ValueError, match="hw_sib_f16"):
        inference_utils.extract_descriptors(crops, size=(96, 72), hw_sib_f16="on")
    for arch in ("seres18", "seres18_hw", "swin"):
        with pytest.raises(ValueError, match="hw_sib_f16.*cares18_hw"):
            reid_inference.inference_efficient(eng, crops, 1, arch=arch, hw_sib_f16=True)
        with pytest.raises(ValueError, match="hw_sib_f16.*cares18_hw"):
            reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch=arch, hw_sib_f16=True)
    with pytest.raises(ValueError, match="hw_ema"):                        # emares18_hw keeps requiring hw_ema=True
        reid_inference.inference_efficient(eng, crops, 1, arch="emares18_hw", size=(96, 72), hw_sib_f16=True)
    for arch, kw in (("cares18_hw", {}), ("emares18_hw", {"hw_ema": True})):
        for extra in ({"hw_precision": "f16x3"}, {"hw_f16": True}):
            with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision.*hw_f16"):
                reid_inference.inference_efficient(eng, crops, 1, arch=arch, size=(96, 72), hw_sib_f16=True, **kw, **extra)
            with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision.*hw_f16"):
                reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch=arch, size=(96, 72), hw_sib_f16=True,
                                             **kw, **extra)
        with pytest.raises(ValueError, match="hw_sib_f16"):
            reid_inference.inference_efficient(eng, crops, 1, arch=arch, size=(96, 72), hw_sib_f16=2, **kw)
        with pytest.raises(ValueError):                                    # a bad size still raises, before the engine
            reid_inference.inference_efficient(eng, crops, 1, arch=arch, size=(31, 72), hw_sib_f16=True, **kw)
        with pytest.raises(ValueError, match="hw_f16.*seres18_hw"):        # hw_f16 on a sibling raises as before
            reid_inference.inference_efficient(eng, crops, 1, arch=arch, size=(96, 72), hw_f16=True, **kw)


def test_extractor_and_model_rules(monkeypatch):
    sds = {a: make(0) for a, make in MAKE_SD.items()}
    se = synth.seres18_state_dict(0)

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    monkeypatch.delenv("REID_PRECISION", raising=False)
    for sd in sds.values():
        for kw in ({}, {"precision": "f16"}, {"precision": "f32"}):
            with pytest.raises(_Stop):                                     # the keyword alone is enough: the next step is the engine
                Extractor(sd, size=(64, 128), hw_sib_f16=True, **kw)
        with pytest.raises(ValueError):                                    # without it the existing rule holds
            Extractor(sd, size=(64, 128))
        with pytest.raises(ValueError, match="hw_sib_f16"):
            Extractor(sd, size=(64, 128), hw_sib_f16="yes")
        with pytest.raises(ValueError, match="hw_sib_f16.*hw_f16"):
            Extractor(sd, size=(64, 128), hw_sib_f16=True, hw_f16=True)
        with pytest.raises(ValueError, match="hw_f16.*seres18_ibn"):       # hw_f16 on a sibling raises as before
            Extractor(sd, size=(64, 128), precision="f32", hw_f16=True)
        with pytest.raises(ValueError):
            Extractor(sd, size=(31, 128), hw_sib_f16=True)
    with pytest.raises(ValueError, match="hw_sib_f16.*cares18_ibn"):
        Extractor(se, size=(64, 128), hw_sib_f16=True)
    with pytest.raises(ValueError, match="hw_sib_f16"):
        Extractor(synth.swin_state_dict(0), hw_sib_f16=True)
    for factory in (cares18_ibn, emares18_ibn):
        assert factory(num_classes=5)._hw_sib_f16 is False and factory(num_classes=5, hw_sib_f16=True)._hw_sib_f16 is True
        with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision"):
            factory(num_classes=5, hw_sib_f16=True, hw_precision="f16x3")
        with pytest.raises(ValueError, match="hw_f16"):                    # as before
            factory(num_classes=5, hw_f16=True)
        with pytest.raises(ValueError, match="hw_f16"):
            factory(num_classes=5, hw_sib_f16=True, hw_f16=True)
        with pytest.raises(ValueError, match="hw_sib_f16"):
            factory(num_classes=5, hw_sib_f16=3)
        with pytest.raises(ValueError):                                    # a bad size is refused before the engine
            factory(num_classes=5, hw_sib_f16=True)(np.zeros((1, 3, 31, 72), np.float32))
    for factory in (seres18_ibn, swin_t):
        with pytest.raises(ValueError, match="hw_sib_f16"):
            factory(num_classes=5, hw_sib_f16=True)
    from reid_amd.models import build_model
    for name in ("cares18_ibn", "emares18_ibn"):
        assert build_model(name, 5, loss="triplet", pretrained=False, hw_sib_f16=True)._hw_sib_f16 is True
        with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision"):
            build_model(name, 5, loss="triplet", pretrained=False, hw_sib_f16=True, hw_precision="f16x3")
    for name in ("seres18_ibn", "swin_transformer"):
        with pytest.raises(ValueError, match="hw_sib_f16"):
            build_model(name, 5, pretrained=False, hw_sib_f16=True)


def test_stream_rules():
    blob = np.zeros(4, np.float32)
    for cls, extra in ((CameraStream, ()), (MultiCameraStream, (2,)), (LookaheadCameraStream, ())):
        for arch in ("seres18", "swin", "seres18_hw"):
            with pytest.raises(ValueError, match="hw_sib_f16"):
                cls(blob, "", *extra, arch=arch, hw_sib_f16=True)
        with pytest.raises(ValueError, match="hw_ema"):                    # emares18_hw keeps requiring hw_ema=True
            cls(blob, "", *extra, arch="emares18_hw", size=(128, 64), hw_sib_f16=True)
        for arch, kw in (("cares18_hw", {}), ("emares18_hw", {"hw_ema": True})):
            with pytest.raises(ValueError, match="hw_sib_f16.*hw_precision"):
                cls(blob, "", *extra, arch=arch, size=(128, 64), hw_sib_f16=True, hw_precision="f16x3", **kw)
            with pytest.raises(ValueError, match="hw_sib_f16.*hw_f16"):
                cls(blob, "", *extra, arch=arch, size=(128, 64), hw_sib_f16=True, hw_f16=True, **kw)
            with pytest.raises(ValueError, match="hw_sib_f16"):
                cls(blob, "", *extra, arch=arch, size=(128, 64), hw_sib_f16="x", **kw)
            with pytest.raises(ValueError):
                cls(blob, "", *extra, arch=arch, size=(31, 64), hw_sib_f16=True, **kw)
            with pytest.raises(ValueError, match="hw_f16"):                # hw_f16 on a sibling raises as before
                cls(blob, "", *extra, arch=arch, size=(128, 64), hw_f16=True, **kw)
