"""Host side of CARes18-IBN at any input size (no GPU): the float64 oracle of the TripletAttention tail (tests/anysize_ca_ref.py) against the
module as oracle/seres18.py states it in torch, the fp32 emulation of the kernels' documented order under the derived bound, seven mutations
that each leave it, the side library's kernel list and independence, the declared / bound / exported surface, the Python rules up to the
first device call, and the fixture's own shape."""
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
import anysize_ca_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize_ca.so")
SIDE_SYMBOLS = ("anysize_ca_workspace_bytes", "anysize_ca_tail")
MUTATIONS = ("biased", "swap_channels", "swap_cw_hc", "transposed_plane", "replicate", "third_on_two", "shortcut_first")
IDS = ["%dx%dx%d" % c for c in ref.CASES]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def table():
    """case -> (y, sc, prm, oracle, bounds) of the "bn" family, n = 2: computed once, shared, never written to."""
    out = {}
    for k, case in enumerate(ref.CASES):
        y, sc = ref.operands(case, 2, "bn")
        prm = ref.make_prm(k)
        out[case] = (y, sc, prm, ref.tail(y, sc, prm), ref.bounds(y, sc, prm))
    return out


# ---------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("case", ref.CASES[:4], ids=IDS[:4])
def test_oracle_equals_the_module_in_float64(case):
    """TripletAttention as oracle/seres18.py restates it with torch (ZPool by torch.std / torch.mean on permuted views, F.conv2d with
    padding 3, an eval-mode BatchNorm2d(1)) in float64 with random weights and running statistics, then relu(. + shortcut)."""
    h, w, c = case
    rng = np.random.default_rng(h * 100 + c)
    y, sc = ref.operands(case, 2, "bn", seed=5)
    sd, prm = {}, np.empty((3, 100), np.float64)
    for row, gate in enumerate(ref.GATE_ORDER):
        wt = rng.normal(0, 0.2, (1, 2, 7, 7))
        gamma, beta, mean, var = rng.uniform(0.5, 1.5), rng.normal(0, 0.3), rng.normal(0, 0.3), rng.uniform(0.5, 2.0)
        pre = "t.%s.conv" % gate
        sd[pre + ".conv.weight"] = torch.from_numpy(wt)
        for key, v in (("weight", gamma), ("bias", beta), ("running_mean", mean), ("running_var", var)):
            sd[pre + ".bn." + key] = torch.tensor([v], dtype=torch.float64)
        scale = gamma / np.sqrt(var + seres18.BN_EPS)
        prm[row, :98], prm[row, 98], prm[row, 99] = wt.reshape(98), scale, beta - mean * scale
    yt = torch.from_numpy(y.astype(np.float64)).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        want = torch.relu(seres18._triplet(sd, "t", yt) + torch.from_numpy(sc.astype(np.float64)).permute(0, 3, 1, 2))
    want = want.permute(0, 2, 3, 1).numpy()
    got, maps, gates = ref.tail(y, sc, prm)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert maps.shape == (2, 2 * ref.per_image(h, w, c)) and gates.shape == (2, ref.per_image(h, w, c))


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_emulation_of_the_documented_order_stays_inside_the_bound(case, family):
    y, sc = ref.operands(case, 2, family)
    prm = ref.make_prm(ref.CASES.index(case))
    want = ref.tail(y, sc, prm)
    got = ref.emulate(y, sc, prm)
    for name, g, w_, b in zip(("out", "maps", "gates"), got, want, ref.bounds(y, sc, prm)):
        assert (b > 0).all() and np.isfinite(b).all()
        worst = float((np.abs(g.astype(np.float64) - w_) / b).max())
        print("%s %s %s: err / bound %.3g, largest bound %.3g" % (case, family, name, worst, b.max()))
        assert worst <= 1.0, (name, worst)
    assert ref.bounds(y, sc, prm)[0].max() < 1e-3
    if family == "const":                                                   # every row of W pixels constant: the hc plane's std is exactly 0
        h, w, c = case
        o = 2 * h * w + 2 * c * w
        assert (want[1][:, o:o + h * c] == 0).all() and (want[1][:, :h * w] > 0).all()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_subtly_wrong_tail_leaves_the_bound(table, mutation):
    """biased variance; mean and std channels swapped; cw and hc weights swapped; the hc plane indexed transposed; replicate instead of
    zero padding; 1/3 on two of three terms; the shortcut added before the 1/3 - each more than ten bounds away on at least one case."""
    caught = []
    for case in ref.CASES:
        y, sc, prm, (out, _, _), (b_out, _, _) = table[case]
        wrong, _, _ = ref.tail(y, sc, prm, **{mutation: True})
        if (np.abs(wrong - out) > 10 * b_out).any():
            caught.append(case)
    print(mutation, "caught on", caught)
    assert caught, mutation + " would pass on every case"


# ---------------------------------------------------------------------------------------------- 2. the side library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_ca.so holds the kernels of tests/golden/kernels_anysize_ca.json by name, none with scratch or AGPRs, none over the
    list's VGPRs or LDS; the product library does not name the file among what it needs; it needs no library of the project and loads on
    its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_ca.json")))
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
    lib.anysize_ca_workspace_bytes.restype = ctypes.c_size_t
    assert lib.anysize_ca_workspace_bytes(3, 56, 67, 64) == 3 * 3 * ref.per_image(56, 67, 64) * 4
    for bad in ((0, 8, 8, 64), (1, 1, 8, 64), (1, 8, 129, 64), (1, 8, 8, 96), (1, 8, 8, 1024)):
        assert lib.anysize_ca_workspace_bytes(*bad) == 0, bad


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    sym = "reid_ctx_set_hw_siblings"
    assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    dbg = _ffi.debug_lib()
    sym = "reid_debug_any_ca_tail"
    assert sym + "(" in dbg_hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(dbg, sym)
    assert '"any_ca"' in dbg_hdr
    for name in ("debug_any_ca_tail", "set_hw_siblings", "hw_siblings_scope"):
        assert callable(getattr(Engine, name))
    assert isinstance(Engine.hw_siblings, property)


# ---------------------------------------------------------------------------------------------- 3. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    embed_dim, num_class = 512, 751
    PIL_MAX_SIDE = Engine.PIL_MAX_SIDE

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_hw_siblings_values():
    eng = _NoDevice()
    for v, want in ((False, 0), (True, 1), (0, 0), (1, 1), (np.bool_(True), 1), (np.int32(1), 1)):
        assert Engine.hw_siblings_value(v) == want
    for bad in (2, -1, "on", None, 1.0, (1,)):
        with pytest.raises(ValueError):
            Engine.hw_siblings_value(bad)
        with pytest.raises(ValueError):
            Engine.set_hw_siblings(eng, bad)                               # before the C ABI is reached
        with pytest.raises(ValueError):
            cares18_ibn(num_classes=5, hw_siblings=bad)
        with pytest.raises(ValueError):
            Extractor(synth.cares18_state_dict(0), size=(64, 128), precision="f32", hw_siblings=bad)

    class _Fresh:
        pass
    assert Engine.hw_siblings.fget(_Fresh()) is False


def test_model_rules(monkeypatch):
    x = np.zeros((1, 3, 96, 72), np.float32)
    with pytest.raises(ValueError, match="seres18_ibn"):                   # without the keyword: what it raised before
        cares18_ibn(num_classes=5)(x)
    with pytest.raises(ValueError, match="seres18_ibn"):
        emares18_ibn(num_classes=5)(x)
    with pytest.raises(ValueError, match="hw_siblings"):
        seres18_ibn(num_classes=5, hw_siblings=True)
    with pytest.raises(ValueError, match="hw_siblings"):
        emares18_ibn(num_classes=5, hw_siblings=True)
    with pytest.raises(ValueError, match="hw_siblings"):
        build_model("seres18_ibn", 5, loss="triplet", pretrained=False, hw_siblings=True)
    with pytest.raises(ValueError, match="hw_siblings"):
        build_model("swin_transformer", 5, pretrained=False, hw_siblings=True)
    model = build_model("cares18_ibn", 5, loss="triplet", pretrained=False, hw_siblings=True)
    assert model._hw_siblings and not cares18_ibn(num_classes=5)._hw_siblings
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


def test_extractor_rules(monkeypatch):
    ca, ema = synth.cares18_state_dict(0), synth.emares18_state_dict(0)

    class _Stop(Exception):
        pass

    def no_engine(device=0):
        raise _Stop()
    import reid_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    for precision in ("f32", "f16x3"):
        with pytest.raises(_Stop):
            Extractor(ca, size=(64, 128), precision=precision, hw_siblings=True)
    with pytest.raises(ValueError, match="f32"):                           # the arithmetic is asked for by name, as for seres18_ibn
        Extractor(ca, size=(64, 128), hw_siblings=True)
    with pytest.raises(ValueError):
        Extractor(ca, size=(64, 128), precision="f16", hw_siblings=True)
    with pytest.raises(ValueError):                                        # without the keyword: refused as before
        Extractor(ca, size=(64, 128), precision="f32")
    with pytest.raises(ValueError, match="emares18_ibn"):
        Extractor(ema, size=(64, 128), precision="f32", hw_siblings=True)
    with pytest.raises(ValueError):
        Extractor(ca, size=(64, 1000), precision="f32", hw_siblings=True)


def test_chain_and_stream_rules():
    eng = _NoDevice()
    assert "cares18_hw" in reid_inference.ARCHS and "seres18_hw" in reid_inference.ARCHS
    crops = [np.zeros((9, 7, 3), np.uint8)]
    lab = np.zeros(1, np.int64)
    with pytest.raises(ValueError, match="size"):
        reid_inference.inference_efficient(eng, crops, 1, arch="cares18_hw")                       # uint8 images need their target
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, np.zeros((2, 3, 20, 20), np.float32), 1, arch="cares18_hw")
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, arch="cares18_hw", size=(31, 72))
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, arch="cares18_hw", size=(96, 72), hw_precision="f16")
    with pytest.raises(ValueError):
        reid_inference.inference_efficient(eng, crops, 1, arch="cares18_hw", size=(96, 72), strong_offsets=np.full((1, 2), 40), pad=10)
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="cares18_hw", size=(600, 72))
    with pytest.raises(ValueError):
        reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch="cares18_hw", size=(96, 72), use_side=True)
    with pytest.raises(ValueError, match="arch"):
        reid_inference.inference_efficient(eng, crops, 1, arch="emares18_hw", size=(96, 72))
    for cls in (tracking.CameraStream, tracking.MultiCameraStream, tracking.LookaheadCameraStream):
        extra = (2,) if cls is tracking.MultiCameraStream else ()
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, arch="cares18_hw", size=(31, 64))
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, arch="cares18_hw", size=(128, 64), hw_precision="f16")
        with pytest.raises(ValueError):
            cls(b"", {}, *extra, arch="cares18_hw", size=(128, 64), mean_std=((0.5,) * 3, (0.0,) * 3))
        with pytest.raises(ValueError, match="arch"):
            cls(b"", {}, *extra, arch="emares18_hw", size=(128, 64))
    tracking._check_arch("cares18_hw", (128, 64), None, "f16x3")


# ---------------------------------------------------------------------------------------------- 4. the fixture
def test_fixture_holds_the_three_cases(golden_dir):
    """tests/golden/anysize_ca.npz: seeds, sizes, the eight block taps, embeddings and logits of three cases of three images, and the
    reference's own float32-against-float64 figures, each at most half of the limit tests/test_gpu_anysize_ca.py applies."""
    path = os.path.join(golden_dir, "anysize_ca.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    assert int(z["n_cases"]) == 3 and int(z["weight_seed"]) == 0
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import anysize_ref
    blocks = [b[0] for b in synth.SERES18_BLOCKS]
    for k, (h, w) in enumerate(((64, 32), (96, 72), (224, 268))):
        p = "c%d_" % k
        assert (int(z[p + "h"]), int(z[p + "w"]), int(z[p + "n"])) == (h, w, 3)
        assert z[p + "emb"].shape == (3, 512) and z[p + "logits"].shape == (3, 751)
        shapes = anysize_ref.stage_shapes(h, w)
        for s, name in enumerate(blocks):
            assert tuple(z[p + "shape_" + name]) == (3, shapes[2 + s][2], shapes[2 + s][0], shapes[2 + s][1]), (k, name)
            assert z[p + "tap_" + name].size <= 3 * 8 * 16 * 8 and np.isfinite(z[p + "tap_" + name]).all()
        for key, limit in (("tap", 2e-5), ("cos", 1e-5), ("emb", 2e-5), ("logits", 5e-5)):
            assert 0 <= float(z[p + "ref_self_error_" + key]) <= 0.5 * limit, (k, key)
