"""Host side of EMARes18-IBN at any input size (no GPU): the float64 oracle of the EMA tail (tests/anysize_ema_ref.py) against the module as
oracle/seres18.py states it and against a torch restatement of EMA.forward, the fp32 emulation of the kernels' documented order under the
derived bound, eleven mutations that each leave it, the side library's kernel list and independence, the declared / bound / exported
surface, the Python rules up to the first device call, and the fixture's own shape."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import seres18
from reid_amd import _ffi, reid_inference, synth, tracking
from reid_amd.backbone import cares18_ibn, emares18_ibn, seres18_ibn
from reid_amd.engine import Engine
from reid_amd.extractor import Extractor
from reid_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_ema_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize_ema.so")
SIDE_SYMBOLS = ("anysize_ema_workspace_bytes", "anysize_ema_tail")
IDS = ["%dx%dx%d" % c for c in ref.CASES]
SMALL = ref.CASES[:7]                                                           # the mutations need no 128 x 128 map


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def table():
    """(case, family) -> (y, sc, prm, oracle out, bound of out), n = 1: computed once, shared, never written to."""
    out = {}
    for k, case in enumerate(SMALL):
        for family in ref.FAMILIES:
            y, sc = ref.operands(case, 1, family)
            prm = ref.make_prm(case[2], k)
            out[case, family] = (y, sc, prm, ref.tail(y, sc, prm)["out"], ref.bounds(y, sc, prm)["out"])
    return out


# ---------------------------------------------------------------------------------------------- 1. the oracle
def _state_dict(prm, cg):
    w1, b1, w3, b3, gw, gb = (torch.from_numpy(np.ascontiguousarray(a, np.float64)) for a in ref.unpack_prm(prm, cg))
    return {"e.conv1x1.weight": w1.reshape(cg, cg, 1, 1), "e.conv1x1.bias": b1, "e.conv3x3.weight": w3, "e.conv3x3.bias": b3,
            "e.gn.weight": gw, "e.gn.bias": gb}


def _ema_forward(sd, x, groups=32):
    """EMA.forward restated with torch modules' functional forms, line for line: adaptive pools, conv2d, group_norm, softmax, matmul."""
    import torch.nn.functional as F
    b, c, h, w = x.size()
    group_x = x.reshape(b * groups, -1, h, w)
    x_h = F.adaptive_avg_pool2d(group_x, (h, 1))
    x_w = F.adaptive_avg_pool2d(group_x, (1, w)).permute(0, 1, 3, 2)
    hw = F.conv2d(torch.cat([x_h, x_w], dim=2), sd["e.conv1x1.weight"], sd["e.conv1x1.bias"])
    x_h, x_w = torch.split(hw, [h, w], dim=2)
    x1 = F.group_norm(group_x * x_h.sigmoid() * x_w.permute(0, 1, 3, 2).sigmoid(), c // groups, sd["e.gn.weight"], sd["e.gn.bias"], 1e-5)
    x2 = F.conv2d(group_x, sd["e.conv3x3.weight"], sd["e.conv3x3.bias"], stride=1, padding=1)
    x11 = torch.softmax(F.adaptive_avg_pool2d(x1, (1, 1)).reshape(b * groups, -1, 1).permute(0, 2, 1), -1)
    x12 = x2.reshape(b * groups, c // groups, -1)
    x21 = torch.softmax(F.adaptive_avg_pool2d(x2, (1, 1)).reshape(b * groups, -1, 1).permute(0, 2, 1), -1)
    x22 = x1.reshape(b * groups, c // groups, -1)
    weights = (torch.matmul(x11, x12) + torch.matmul(x21, x22)).reshape(b * groups, 1, h, w)
    return (group_x * weights.sigmoid()).reshape(b, c, h, w)


@pytest.mark.parametrize("case", ref.CASES[:5], ids=IDS[:5])
def test_oracle_equals_the_module_in_float64(case):
    """relu(EMA(y) + shortcut) as oracle/seres18.py states the block (its _ema) and as a torch restatement of EMA.forward gives it, in
    float64 with random parameters."""
    h, w, c = case
    y, sc = ref.operands(case, 2, "normal", seed=5)
    prm = ref.make_prm(c, 40 + h)
    sd = _state_dict(prm, c // 32)
    yt = torch.from_numpy(y.astype(np.float64)).permute(0, 3, 1, 2).contiguous()
    sct = torch.from_numpy(sc.astype(np.float64)).permute(0, 3, 1, 2)
    got = ref.tail(y, sc, prm)
    with torch.no_grad():
        for fn in (lambda: seres18._ema(sd, "e", yt), lambda: _ema_forward(sd, yt)):
            want = torch.relu(fn() + sct).permute(0, 2, 3, 1).numpy()
            assert np.abs(got["out"] - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert got["sig"].shape == (2, h + w, c) and all(got[k].shape == (2, c) for k in ("mu", "rstd", "s1", "s2"))


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_emulation_of_the_documented_order_stays_inside_the_bound(case, family):
    n = ref.BATCHES[case][-1] if case[0] * case[1] <= 4096 else 1
    y, sc = ref.operands(case, n, family)
    prm = ref.make_prm(case[2], ref.CASES.index(case))
    want, got, bound = ref.tail(y, sc, prm, full=True), ref.emulate(y, sc, prm), ref.bounds(y, sc, prm)
    for name in ref.NAMES:
        b = bound[name]
        assert (b > 0).all() and np.isfinite(b).all()
        worst = float((np.abs(got[name].astype(np.float64) - want[name]) / b).max())
        print("%s %s %s: err / bound %.3g, largest bound %.3g" % (case, family, name, worst, b.max()))
        assert worst <= 1.0, (name, worst)
    if family == "const":                                                   # the GroupNorm variance is 0 and x1 is the GroupNorm bias
        gb = ref.unpack_prm(prm, case[2] // 32)[5].astype(np.float64)
        assert want["var"].max() < 1e-25 and np.abs(want["x1"] - gb).max() < 1e-9
    if family == "saturate":
        assert want["sig"].min() < 1e-6 and want["sig"].max() > 1 - 1e-6 and min(want["g"].min(), 1 - want["g"].max()) < 1e-3
    if family == "normal":
        assert bound["out"].max() < 1e-3


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_a_subtly_wrong_tail_leaves_the_bound(table, mutation):
    """Variance over hw - 1; eps 1e-6; the softmax of agp(x1) applied to x1; pool_h and pool_w exchanged (an H != W map); clamped padding;
    the 1x1 bias dropped; the 3 x 3 weight read as [ci][co]; one sigmoid factor dropped; the GroupNorm affine dropped; interleaved channel
    groups; the shortcut added before the gate - each more than ten bounds away on at least one case."""
    caught = []
    for (case, family), (y, sc, prm, out, b_out) in table.items():
        if mutation == "swap_pools" and case[0] == case[1]:
            continue
        wrong = ref.tail(y, sc, prm, **{mutation: True})["out"]
        if (np.abs(wrong - out) > 10 * b_out).any():
            caught.append((case, family))
    print(mutation, "caught on", caught)
    assert caught, mutation + " would pass on every case"


# ---------------------------------------------------------------------------------------------- 2. the side library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_ema.so holds the kernels of tests/golden/kernels_anysize_ema.json by name, none with scratch or AGPRs, none over
    the list's VGPRs or LDS (so none holds a slab of the map); the product library does not name the file among what it needs; it needs no
    library of the project and loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_ema.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values()), {k: v["vgprs"] for k, v in got.items()}
    assert all(v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    lib = ctypes.CDLL(LIB)
    for sym in SIDE_SYMBOLS:
        assert hasattr(lib, sym)
    lib.anysize_ema_workspace_bytes.restype = ctypes.c_size_t
    # (56, 67, 64): 56 * 67 * 16 / 1024 -> 59 slabs, at most one per row -> 56; part [56][3][64] fp64, sig [123][64], small [4][64] fp32
    assert lib.anysize_ema_workspace_bytes(3, 56, 67, 64) == 3 * (56 * 3 * 64 * 8 + (56 + 67) * 64 * 4 + 4 * 64 * 4)
    # (6, 5, 256): 1920 pieces -> 2 slabs of 3 rows
    assert lib.anysize_ema_workspace_bytes(1, 6, 5, 256) == 2 * 3 * 256 * 8 + (6 + 5) * 256 * 4 + 4 * 256 * 4
    assert lib.anysize_ema_workspace_bytes(1, 128, 128, 64) > 0 and lib.anysize_ema_workspace_bytes(65535, 2, 2, 512) > 0
    for bad in ((0, 8, 8, 64), (65536, 8, 8, 64), (1, 1, 8, 64), (1, 8, 129, 64), (1, 8, 8, 96), (1, 8, 8, 1024), (1, 8, 8, 32)):
        assert lib.anysize_ema_workspace_bytes(*bad) == 0, bad


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    sym = "reid_ctx_set_hw_ema"
    assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    dbg = _ffi.debug_lib()
    sym = "reid_debug_any_ema_tail"
    assert sym + "(" in dbg_hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(dbg, sym)
    assert '"any_ema"' in dbg_hdr
    for name in ("debug_any_ema_tail", "set_hw_ema", "hw_ema_scope"):
        assert callable(getattr(Engine, name))
    assert isinstance(Engine.hw_ema, property)


# ---------------------------------------------------------------------------------------------- 3. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    PIL_MAX_SIDE = Engine.PIL_MAX_SIDE

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


class _Recorder:
    """An engine's setting and its scope, without a device: what the chain does with hw_ema."""
    hw_ema = Engine.hw_ema
    hw_ema_scope = Engine.hw_ema_scope

    def __init__(self):
        self.calls = []

    def set_hw_ema(self, on):
        self.calls.append(bool(on))
        self._hw_ema = bool(on)


def test_hw_ema_values():
    eng = _NoDevice()
    for v, want in ((False, 0), (True, 1), (0, 0), (1, 1), (np.bool_(True), 1), (np.int32(1), 1)):
        assert Engine.hw_ema_value(v) == want
    for bad in (2, -1, "on", None, 1.0, (1,)):
        with pytest.raises(ValueError):
            Engine.hw_ema_value(bad)
        with pytest.raises(ValueError):
            Engine.set_hw_ema(eng, bad)                                    # before the C ABI is reached
        with pytest.raises(ValueError):
            emares18_ibn(num_classes=5, hw_ema=bad)
        with pytest.raises(ValueError):
            Extractor(synth.emares18_state_dict(0), size=(64, 128), precision="f32", hw_ema=bad)

    class _Fresh:
        pass
    assert Engine.hw_ema.fget(_Fresh()) is False
    rec = _Recorder()
    with rec.hw_ema_scope(None):
        assert rec.calls == []
    with rec.hw_ema_scope(True):
        assert rec.hw_ema is True
    assert rec.calls == [True, False] and rec.hw_ema is False
    rec.set_hw_ema(True)
    with rec.hw_ema_scope(True):
        pass
    assert rec.hw_ema is True                                              # what it was before comes back, on included


def test_model_rules(monkeypatch):
    x = np.zeros((1, 3, 96, 72), np.float32)
    with pytest.raises(ValueError, match="seres18_ibn"):                   # without the keyword: what it raised before
        emares18_ibn(num_classes=5)(x)
    with pytest.raises(ValueError, match="hw_siblings"):                   # hw_siblings is not its keyword: what it raised before
        emares18_ibn(num_classes=5, hw_siblings=True)
    for other in (seres18_ibn, cares18_ibn):
        with pytest.raises(ValueError, match="hw_ema"):
            other(num_classes=5, hw_ema=True)
    with pytest.raises(ValueError, match="hw_ema"):
        build_model("seres18_ibn", 5, loss="triplet", pretrained=False, hw_ema=True)
    with pytest.raises(ValueError, match="hw_ema"):
        build_model("cares18_ibn", 5, loss="triplet", pretrained=False, hw_ema=True)
    with pytest.raises(ValueError, match="hw_ema"):
        build_model("swin_transformer", 5, pretrained=False, hw_ema=True)
    model = build_model("emares18_ibn", 5, loss="triplet", pretrained=False, hw_ema=True)
    assert model._hw_ema and not emares18_ibn(num_classes=5)._hw_ema and not model._hw_siblings
    with pytest.raises(ValueError):                                        # the size range still holds
        model(np.zeros((1, 3, 31, 72), np.float32))

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.backbone as backbone_mod
    monkeypatch.setattr(backbone_mod, "get_engine", no_engine)
    with pytest.raises(_Stop):                                             # the argument checks pass: the next step is the engine
        model(x)
    with pytest.raises(_Stop):
        emares18_ibn(num_classes=5, hw_ema=True, hw_precision="f16x3")(x)


def test_extractor_rules(monkeypatch):
    ca, ema, se = synth.cares18_state_dict(0), synth.emares18_state_dict(0), synth.seres18_state_dict(0)

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    for precision in ("f32", "f16x3"):
        with pytest.raises(_Stop):
            Extractor(ema, size=(64, 128), precision=precision, hw_ema=True)
    with pytest.raises(ValueError, match="f32"):                           # the arithmetic is asked for by name, as for seres18_ibn
        Extractor(ema, size=(64, 128), hw_ema=True)
    with pytest.raises(ValueError):
        Extractor(ema, size=(64, 128), precision="f16", hw_ema=True)
    with pytest.raises(ValueError, match="emares18_ibn"):                  # without the keyword: refused as before
        Extractor(ema, size=(64, 128), precision="f32")
    with pytest.raises(ValueError, match="emares18_ibn"):                  # hw_siblings does not open it: what it raised before
        Extractor(ema, size=(64, 128), precision="f32", hw_siblings=True)
    with pytest.raises(ValueError):
        Extractor(ema, size=(64, 1000), precision="f32", hw_ema=True)
    for other in (ca, se):
        with pytest.raises(ValueError, match="hw_ema"):
            Extractor(other, size=(64, 128), precision="f32", hw_ema=True)


def test_chain_and_stream_rules():
    eng = _NoDevice()
    assert "emares18_hw" not in reid_inference.ARCHS                       # the name alone stays an unknown one
    crops = [np.zeros((9, 7, 3), np.uint8)]
    lab = np.zeros(1, np.int64)
    kw = dict(arch="emares18_hw", hw_ema=True)
    with pytest.raises(ValueError, match="arch"):                          # without the keyword: what it raises today
        reid_inference.inference_efficient(eng, crops, 1, arch="emares18_hw", size=(96, 72))
    with pytest.raises(ValueError, match="arch"):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="emares18_hw", size=(96, 72))
    with pytest.raises(ValueError, match="arch"):
        reid_inference.inference_efficient(eng, crops, 1, arch="emares18_hw", size=(96, 72), hw_ema=False)
    for other in ("seres18", "seres18_hw", "cares18_hw", "swin"):          # the keyword on another arch
        with pytest.raises(ValueError, match="hw_ema"):
            reid_inference.inference_efficient(eng, crops, 1, arch=other, size=(96, 72), hw_ema=True)
    with pytest.raises(ValueError, match="hw_ema"):
        reid_inference.inference_efficient(eng, crops, 1, size=(96, 72), hw_ema=2, arch="emares18_hw")
    with pytest.raises(ValueError, match="size"):
        reid_inference.inference_efficient(eng, crops, 1, **kw)                                    # uint8 images need their target
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 20, 20), np.float32), 1, **kw)
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, size=(31, 72), **kw)
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, size=(96, 72), hw_precision="f16", **kw)
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, size=(96, 72), strong_offsets=np.full((1, 2), 40), pad=10, **kw)
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, size=(600, 72), **kw)
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, size=(96, 72), use_side=True, **kw)
    for cls in (tracking.CameraStream, tracking.MultiCameraStream, tracking.LookaheadCameraStream):
        extra = (2,) if cls is tracking.MultiCameraStream else ()
        with pytest.raises(ValueError, match="arch"):                      # without the keyword: what it raises today
            cls(b"", {}, *extra, arch="emares18_hw", size=(128, 64))
        with pytest.raises(ValueError, match="hw_ema"):
            cls(b"", {}, *extra, arch="cares18_hw", size=(128, 64), hw_ema=True)
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, size=(31, 64), **kw)
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, size=(128, 64), hw_precision="f16", **kw)
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, size=(128, 64), mean_std=((0.5,) * 3, (0.0,) * 3), **kw)
    tracking._check_arch("emares18_hw", (128, 64), None, "f16x3", True)
    assert "hw_ema" not in tracking.ShardedCameraStream.__init__.__code__.co_varnames    # it stays at 256 x 128


def test_the_chain_scopes_the_setting(monkeypatch):
    """inference_efficient(arch="emares18_hw", hw_ema=True): the setting goes on for the device work - which runs as "seres18_hw" - and
    comes back after it, also when the work raises."""
    class _Stop(Exception):
        pass

    class _Eng(_Recorder):
        embed_dim, num_class = 512, 751
        hw_precision_scope = Engine.hw_precision_scope
        hw_siblings_scope = Engine.hw_siblings_scope

    seen = []

    def work(engine, images, d_out, flip, bs, arch, view_index, size, width, strong_offsets=None, pad=10):
        seen.append((arch, engine.hw_ema))
        raise _Stop()
    monkeypatch.setattr(reid_inference, "_inference_u8", work)
    eng = _Eng()
    with pytest.raises(_Stop):
        reid_inference.inference_efficient(eng, [np.zeros((9, 7, 3), np.uint8)], 1, arch="emares18_hw", hw_ema=True, size=(96, 72))
    assert seen == [("seres18_hw", True)] and eng.calls == [True, False] and eng.hw_ema is False


# ---------------------------------------------------------------------------------------------- 4. the fixture
def test_fixture_holds_the_three_cases(golden_dir):
    """tests/golden/anysize_ema.npz: seeds, sizes, the eight block taps, embeddings and logits of three cases of three images, and the
    reference's own float32-against-float64 figures, each at most half of the limit tests/test_gpu_anysize_ema.py applies."""
    path = os.path.join(golden_dir, "anysize_ema.npz")
    assert os.path.getsize(path) < 1000000
    z = np.load(path)
    assert int(z["n_cases"]) == 3 and int(z["weight_seed"]) == 0
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import anysize_ref
    blocks = [b[0] for b in synth.SERES18_BLOCKS]
    for k, (h, w, seed) in enumerate(((64, 32, 11), (96, 72, 12), (224, 268, 13))):
        p = "c%d_" % k
        assert (int(z[p + "h"]), int(z[p + "w"]), int(z[p + "n"]), int(z[p + "seed"])) == (h, w, 3, seed)
        assert z[p + "emb"].shape == (3, 512) and z[p + "logits"].shape == (3, 751)
        shapes = anysize_ref.stage_shapes(h, w)
        for s, name in enumerate(blocks):
            assert tuple(z[p + "shape_" + name]) == (3, shapes[2 + s][2], shapes[2 + s][0], shapes[2 + s][1]), (k, name)
            assert z[p + "tap_" + name].size <= 3 * 8 * 16 * 8 and np.isfinite(z[p + "tap_" + name]).all()
        for key, limit in (("tap", 2e-5), ("cos", 1e-5), ("emb", 2e-5), ("logits", 5e-5)):
            assert 0 <= float(z[p + "ref_self_error_" + key]) <= 0.5 * limit, (k, key)
