"""Host side of the fp32-class distance matrix (no GPU): the side library's kernel list and independence, the declared / bound / exported
surface, the numpy restatement of the split arithmetic on the input families the GPU tests rely on (tests/distmat_x3_ref.py) with the
mutations those families are there to catch, the seeded rank input, and the Python rules up to the first device call."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, distance
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distmat_x3_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_distmat_x3.so")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


# ---------------------------------------------------------------------------------------------- 1. the library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_distmat_x3.so holds the kernels of tests/golden/kernels_distmat_x3.json by name, none with scratch or AGPRs, none over
    the VGPR or LDS cap that two blocks per CU allow; the product library does not name the file among what it needs, the side library
    needs nothing of the project's, and it loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_distmat_x3.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert sorted(spec["vgprs"]) == sorted(want)
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values()), {k: v["vgprs"] for k, v in got.items()}
    assert all(0 < v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_distmat" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    assert hasattr(ctypes.CDLL(LIB), "distmat_x3")


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    for sym in ("reid_distmat_x3", "reid_distmat_x3_dev"):
        assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym), sym
        assert _ffi._SIGS[sym] == _ffi._SIGS[sym.replace("_x3", "")]
    comment = hdr[:hdr.index("int reid_distmat_x3(")].rsplit("/*", 1)[1]
    for word in ("reid/losses/utils.py:12-35", "65504", "31.98", "rank", "REID_K_DIST_GEMM", "libreid_hip_distmat_x3.so"):
        assert word in comment, word


# ---------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_exact_family_is_exact_in_fp32(shape):
    """Every term is a multiple of 0.25 and sum |terms| / 0.25 < 2^24: fp32 accumulation is exact in any order, the three-product value is
    one fp32 number.  Exchanging yq and yh changes (nearly) every output; from 32 columns on so does dropping either cross product; and no
    two rows and no two columns of the result agree, so a lost, repeated or misplaced row or column cannot produce its bits."""
    m, n, d = shape
    x, y = ref.exact_operands(*shape)
    xh, xl = ref.split(x)
    yh, yl = ref.split(y)
    assert set(np.unique(xh)) <= {-1.0, 0.0, 1.0} and set(np.unique(xl)) <= {-0.25, 0.0, 0.25}
    assert set(np.unique(yh)) <= {-1.0, 1.0} and set(np.unique(yl)) <= {-0.25, 0.0, 0.25}
    val, mag = ref.restate(x, y)
    quarters = mag.max() / 0.25
    print("%s: largest sum |terms| / 0.25 = %.3g" % (shape, quarters))
    assert quarters < 2.0 ** 24
    assert np.array_equal(val * 2048.0 * 4.0, np.round(val * 2048.0 * 4.0))
    assert np.array_equal(val.astype(np.float32).astype(np.float64), val)            # one fp32 number
    assert (val != 0).any()
    swapped = float((ref.restate(x, y, swap_qh=True)[0] != val).mean())
    assert swapped > 0.9, swapped
    if d >= 32:
        for drop in ("lh", "hl"):
            changed = float((ref.restate(x, y, drop=drop)[0] != val).mean())
            print("%s: without the %s product %.0f %% of the outputs change" % (shape, drop, 100 * changed))
            assert changed > 0.5
        assert len(np.unique(val, axis=0)) == m and len(np.unique(val.T, axis=0)) == n


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_small_family_needs_f16_subnormals(shape):
    """x ~ N(0, 1) 2^-15: the faithful restatement stays inside the dot product's bound; with f16 subnormals flushed in xh, or in xl', it
    lies outside it."""
    x, y = ref.small_operands(*shape)
    want, b = ref.oracle(x, y, ref.METRIC_DOT)

    def share(**kw):
        return float((np.abs(ref.restate(x, y, **kw)[0] - want) / b).max())
    good, hi, lo = share(), share(flush_hi=True), share(flush_lo=True)
    print("%s: err / bound faithful %.3g, xh flushed %.3g, xl' flushed %.3g" % (shape, good, hi, lo))
    assert good < 1.0 and hi > 1.0 and lo > 1.0


@pytest.mark.parametrize("name", sorted(ref.METRICS))
def test_restatement_is_inside_every_metrics_bound(name):
    """The float64 restatement through the float64 formulas is inside each metric's bound on the cancellation input (the bound has room
    for the kernel's fp32 accumulation on top)."""
    metric = ref.METRICS[name]
    x, y = ref.random_operands(200, 260, 160, unit=name.startswith("COS"))
    dot = ref.restate(x, y)[0]
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    rs, cq = (x64 * x64).sum(1)[:, None], (y64 * y64).sum(1)[None, :]
    got = {"L2": np.sqrt(np.maximum(rs + cq - 2 * dot, 1e-12)), "L2SQR": rs + cq - 2 * dot, "COS_HALF": (1 - dot / np.sqrt(rs * cq)) / 2,
           "COS": 1 - dot / np.sqrt(rs * cq), "DOT": dot}[name]
    share, ok = ref.check(got, x, y, metric)
    print("%s: restatement err / bound %.3g" % (name, share))
    assert ok and share < 0.5


def test_the_float64_bound_alone_misses_a_dropped_product():
    """Why the exact family exists: on random operands of the descriptors' width a dropped xl'.yh stays inside the float64 bound."""
    x, y = ref.random_operands(64, 200, 512)
    want, b = ref.oracle(x, y, ref.METRIC_DOT)
    assert (np.abs(ref.restate(x, y, drop="lh")[0] - want) <= b).all()


def test_rank_input_has_clear_winners():
    """The seeded 64 x 200 x 512 unit rows: the float64 matrix alone leaves out no row - every top-2 gap exceeds the sum of both bounds."""
    x, y = ref.rank_operands()
    assert x.shape == (64, 512) and y.shape == (200, 512)
    for metric in (ref.METRIC_L2SQR, ref.METRIC_COS):
        best, clear = ref.rank_rows(x, y, metric)
        assert clear.all(), (metric, int((~clear).sum()))


def test_tile_rule_and_shapes():
    assert {ref.form_of(s[1]) for s in ref.SHAPES} == {ref.FORM_128x64, ref.FORM_128x128}
    assert ref.form_of(64) == ref.FORM_128x64 and ref.form_of(65) == ref.FORM_128x128
    src = open(os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc", "distmat_x3.hip")).read()
    assert "n <= 64 ? 64 : 128" in src


# ---------------------------------------------------------------------------------------------- 3. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_precision_values(monkeypatch):
    for v, want in ((None, 0), ("f32", 0), ("f16x3", 2)):
        assert Engine.distmat_precision_value(v) == want
    x = np.zeros((2, 4), np.float32)
    import reid_amd.engine as engine_mod

    def no_engine(device=0):
        raise AssertionError("reached the device")
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    monkeypatch.setattr(distance, "get_engine", no_engine)
    for bad in ("f16", "F16X3", "fp32", "", 0, 2, 1.0, True, ("f16x3",)):
        with pytest.raises(ValueError):
            Engine.distmat_precision_value(bad)
        with pytest.raises(ValueError):
            Engine.distmat(_NoDevice(), x, x, _ffi.METRIC_L2, precision=bad)          # before the C ABI is reached
        with pytest.raises(ValueError):
            Engine.distmat_dev(_NoDevice(), 0, 2, 0, 2, 4, _ffi.METRIC_L2, 0, precision=bad)
        for fn in (distance.euclidean_dist, distance.cosine_dist, distance.cosine_distance):
            with pytest.raises(ValueError):
                fn(x, x, precision=bad)                                                # before the engine is made
    for fn in (distance.euclidean_dist, distance.cosine_dist, distance.cosine_distance):
        for ok in (None, "f32", "f16x3"):
            with pytest.raises(AssertionError, match="reached the device"):
                fn(x, x, 0, ok)                                                        # positional (x, y, device, precision)


def test_the_other_matching_calls_take_no_precision():
    import inspect
    for fn in (distance.nearest, distance.search_raw_array, distance.IndexFlatL2.__init__, distance.IndexFlatL2.search):
        assert "precision" not in inspect.signature(fn).parameters, fn
    for fn in (distance.euclidean_dist, distance.cosine_dist, distance.cosine_distance):
        assert list(inspect.signature(fn).parameters) == ["x", "y", "device", "precision"]
        assert inspect.signature(fn).parameters["precision"].default is None
    assert inspect.signature(Engine.distmat).parameters["precision"].default is None


def test_which_entry_a_precision_reaches():
    """None and "f32" call reid_distmat - today's call -, "f16x3" reid_distmat_x3, with the same arguments."""
    calls = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append(name)
                return 0
            return fn

    class _Eng:
        lib, h = _Lib(), None
    x = np.zeros((2, 4), np.float32)
    for p in (None, "f32", "f16x3"):
        Engine.distmat(_Eng(), x, x, _ffi.METRIC_COS, precision=p)
        Engine.distmat_dev(_Eng(), 0, 2, 0, 2, 4, _ffi.METRIC_COS, 0, precision=p)
    Engine.distmat(_Eng(), x, x)
    assert calls == ["reid_distmat", "reid_distmat_dev"] * 2 + ["reid_distmat_x3", "reid_distmat_x3_dev", "reid_distmat"]
