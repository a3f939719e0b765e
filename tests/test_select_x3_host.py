"""Host side of the selection with fp32-class candidates (no GPU).  What is held to what: the numpy restatement of the pipeline
(tests/select_x3_ref.py) to the plain (value, column) selection of the float64 oracle, on the inputs the GPU tests run; three mutations -
a proof without B, a T taken from the merged list only (it forgets the filter's threshold, and the last values of the full tile lists),
ties to the higher column - each to a wrong answer on an input built for
it; the device's bound B, restated from its closed form, to the sum of the bounds tests/distmat_x3_ref.py and tests/matching_ref.py
derive; the side library's kernels to tests/golden/kernels_select_x3.json; the new symbols to the headers, the bindings and the
libraries; and the Python rules to a stand-in engine that raises on any device call."""
import ctypes
import inspect
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
import distmat_x3_ref as x3  # noqa: E402
import matching_ref as mref  # noqa: E402
import select_x3_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_select_x3.so")
CSRC = os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


# ---------------------------------------------------------------------------------------------- 1. the library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_select_x3.so holds the kernels of tests/golden/kernels_select_x3.json by name and register count, none with scratch or
    AGPRs, none over the LDS cap that two blocks per CU allow; the product library does not need the file, the side library needs
    nothing of the project's, and it loads on its own, without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    spec = json.load(open(os.path.join(golden_dir, "kernels_select_x3.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert {k: v["vgprs"] for k, v in got.items()} == spec["vgprs"]
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values())
    assert all(v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_select" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "select_x3") and hasattr(lib, "select_x3_ws_bytes")
    lib.select_x3_ws_bytes.restype = ctypes.c_size_t
    small, market, rerank = (lib.select_x3_ws_bytes(m, n) for m, n in ((5, 3), (3368, 15913), (19281, 19281)))
    assert 64 < small < 8192 and market < 128 << 20 and rerank <= 256 << 20       # a share of the m x n matrix, capped


def test_the_product_library_gained_no_kernel_and_the_matrix_file_is_untouched(built, golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    assert not [n for n in so_kernels.kernels(_ffi.LIB_PATH) if "x3_kernel" in n and "cand" in n]
    src = open(os.path.join(CSRC, "select_x3.hip")).read()
    assert '#include "distmat_x3.h"' not in src and "select_x3" not in open(os.path.join(CSRC, "distmat_x3.hip")).read()
    assert "n <= 64 ? 64 : 128" in src                                          # the tile rule of distmat_x3.h, of n alone
    for word in ("spin", "while (atomic", "__threadfence", "volatile"):           # launches are ordered by the stream only
        assert word not in src, word


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    for sym in ("reid_argmin_rows_x3", "reid_argmin_rows_x3_dev", "reid_knn_x3", "reid_knn_x3_dev"):
        assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym), sym
        assert _ffi._SIGS[sym] == _ffi._SIGS[sym.replace("_x3", "")]
    comment = hdr[:hdr.index("int reid_argmin_rows_x3(")].rsplit("/*", 1)[1]
    for word in ("evaluate.py:58-63", "bits of reid_argmin_rows", "65504", "31.98", "libreid_hip_select_x3.so", "whatever m, n"):
        assert word in comment, word
    comment = hdr[:hdr.index("int reid_knn_x3(")].rsplit("/*", 1)[1]
    for word in ("faiss_utils.py:56-139", "bits of reid_knn", "1 <= k <= 24", "whatever nq, nb"):
        assert word in comment, word
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    assert "int reid_debug_select_x3(" in dbg_hdr and "reid_debug_select_x3" in _ffi.DEBUG_EXPORTS
    assert hasattr(ctypes.CDLL(_ffi.DEBUG_LIB_PATH), "reid_debug_select_x3")


# ---------------------------------------------------------------------------------------------- 2. the restatement
CASES = [(s, u) for s in ref.SHAPES for u in (False, True)]


@pytest.mark.parametrize("shape,unit", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_restated_pipeline_selects_what_the_oracle_selects(shape, unit):
    """Approximate values from the restated three-product arithmetic, exact values from the float64 oracle: on the sets of the GPU
    tests the pipeline returns the plain selection of the exact values on every row, every row's float64 gap is clear, and no row
    takes the fallback - the condition the GPU test asserts of the device."""
    for name, metric in sorted(ref.METRICS.items()):
        for k in ((1, 5, 24) if metric == ref.METRIC_L2SQR else (1,)):
            x, y, clear, gap, b = ref.float64_case(shape, metric, unit, k)
            assert clear.all(), (name, k, int((~clear).sum()))
            a = ref.approx_values(x, y, metric)
            e = mref.oracle(x, y, metric)
            D, I, redo = ref.pipeline(a, e, k, ref.row_bound(x, y, metric), metric)
            wD, wI = ref.plain_select(e, k)
            assert np.array_equal(I, wI) and np.array_equal(D, wD), (name, k)
            assert not redo.any(), (name, k, int(redo.sum()))


def test_adversarial_rows_are_recomputed_and_ties_go_down():
    assert {j // 128 for j in (10, 140)} == {0, 1} and {j // 128 for j in (37, 290)} == {0, 2}
    for name, metric in sorted(ref.METRICS.items()):
        x, y, near = ref.adversarial_operands(negate=name == "DOT")
        a, e = ref.approx_values(x, y, metric), mref.oracle(x, y, metric)
        B = ref.row_bound(x, y, metric)
        for r, cols in near.items():
            v = np.sort(mref.oracle(x, y, ref.METRIC_L2SQR if metric == ref.METRIC_L2 else metric)[r, cols])
            assert len(cols) == 40 > ref.KK and v[-1] - v[0] < B[r], (name, r)          # 40 near-ties inside B
        for k in ((1, 5, 24) if metric == ref.METRIC_L2SQR else (1,)):
            D, I, redo = ref.pipeline(a, e, k, B, metric)
            wD, wI = ref.plain_select(e, k)
            assert np.array_equal(I, wI), (name, k)
            assert redo[2:].all(), (name, k, redo)
            assert I[0, 0] == 10 and I[1, 0] == 37


def test_the_sample_rule():
    assert [ref.sample_of(n) for n in (1, 300, 512, 4096, 15913, 19281, 100000)] == [1, 300, 512, 512, 1024, 1280, 6272]
    src = open(os.path.join(CSRC, "select_x3.hip")).read()
    assert "(n / 16 + 127) / 128 * 128" in src and "SELECT_X3_SAMPLE = 512" in open(os.path.join(CSRC, "select_x3.h")).read()


def test_forced_rows_take_the_fallback():
    x, y = x3.random_operands(130, 70, 100)
    a, e = ref.approx_values(x, y, ref.METRIC_COS), mref.oracle(x, y, ref.METRIC_COS)
    D, I, redo = ref.pipeline(a, e, 1, ref.row_bound(x, y, ref.METRIC_COS), ref.METRIC_COS, force_every=3)
    assert np.array_equal(np.flatnonzero(redo), np.arange(0, 130, 3)) and np.array_equal(I, ref.plain_select(e, 1)[1])


# ---------------------------------------------------------------------------------------------- 3. mutations, one per rule
def _bound_input():
    """33 columns, KK = 32 candidates, B = 0.1: column 32 has the largest approximate value (the filter drops it) and the smallest exact
    one; both arithmetics agree within 0.09 everywhere."""
    a = np.array([[1.0] + [1.05 + 0.001 * j for j in range(1, 32)] + [1.09]])
    e = a.copy()
    e[0, 0], e[0, 32] = 1.08, 1.0
    assert np.abs(a - e).max() < 0.1
    return a, e, np.array([0.1])


def test_mutation_a_proof_that_ignores_the_bound():
    a, e, B = _bound_input()
    D, I, redo = ref.pipeline(a, e, 1, B)
    assert I[0, 0] == 32 and redo[0], "the faithful pipeline cannot prove the row and recomputes it"
    D, I, redo = ref.pipeline(a, e, 1, B, ignore_bound=True)
    assert I[0, 0] == 1 and not redo[0], "without B the row counts as proven and the answer is wrong"


def test_mutation_a_threshold_from_the_merged_list_only():
    a, e, B = _bound_input()
    D, I, redo = ref.pipeline(a, e, 1, B, merged_only=True)
    assert I[0, 0] == 1 and not redo[0], "the merge dropped nothing, so T = +inf: the column the FILTER dropped is forgotten"
    # and with a dropped key: T has to be the smaller of the two
    a2 = np.concatenate([a, [[1.0805]]], 1)                                     # column 33: group 33, below thr0 = the 32nd group minimum
    e2 = np.concatenate([e, [[1.0805]]], 1)
    D, I, redo = ref.pipeline(a2, e2, 1, B)
    assert I[0, 0] == 32 and redo[0]


def test_mutation_a_threshold_that_forgets_the_full_tile_lists():
    """700 columns, the threshold from the first 512.  Columns 520 .. 559 - one tile, outside the sample - hold 40 small values: the
    tile's list keeps its 32 smallest, the last of them (0.531) bounds the eight it left out, and one of those (column 555) has the
    smallest exact value.  From the merged list alone T is the sample's smallest value, about 1, and the row counts as proven."""
    rng = np.random.default_rng(2)
    a = 1.0 + rng.random((1, 700))
    a[0, 520:560] = 0.5 + 0.001 * np.arange(40)
    e = a.copy()
    e[0, 555] = 0.45
    B = np.array([0.1])
    assert np.abs(a - e).max() < B[0]
    D, I, redo = ref.pipeline(a, e, 1, B)
    assert I[0, 0] == 555 and redo[0]
    D, I, redo = ref.pipeline(a, e, 1, B, merged_only=True)
    assert I[0, 0] == 520 and not redo[0]


def test_mutation_ties_to_the_higher_column():
    rng = np.random.default_rng(1)
    a = 1.0 + rng.random((2, 300))
    a[0, 7] = a[0, 200] = 0.5                                                    # two tiles, one value
    a[1, 5], a[1, 150], a[1, 151] = 0.25, 0.5, 0.5
    B = np.full(2, 1e-6)
    D, I, redo = ref.pipeline(a, a, 3, B)
    assert I[0, 0] == 7 and list(I[1]) == [5, 150, 151] and not redo.any()
    D, I, redo = ref.pipeline(a, a, 3, B, higher=True)
    assert I[0, 0] == 200 and list(I[1]) == [5, 151, 150], "a wrong index and a wrong order"


# ---------------------------------------------------------------------------------------------- 4. the bound
def _families(shape):
    yield "exact", x3.exact_operands(*shape)
    yield "random", x3.random_operands(*shape)
    yield "random unit", x3.random_operands(*shape, unit=True)
    yield "small", x3.small_operands(*shape)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_the_device_bound_dominates_both_derivations(shape):
    """B (bound_of, restated in float64 from its closed form of ld, |x_i|^2, max |y|^2 and - cosine - min |y|^2) >= the bound
    tests/distmat_x3_ref.py derives for the fp32-class entry + the bound tests/matching_ref.py derives for the exact entry, on every
    element of the row, with 2^-20 to spare for the device's fp32 evaluation; the random family carries the cancellation rows.  (That B is not idle is
    the GPU test's business: no clear row may be recomputed.)"""
    for fam, (x, y) in _families(shape):
        for name, metric in sorted(ref.METRICS.items()):
            live = np.abs(x).sum(1) > 0 if name.startswith("COS") else np.ones(len(x), bool)    # 0 / 0: no cosine, no bound
            with np.errstate(all="ignore"):
                s = ref.summed_bounds(x, y, metric)[live].max(1)
            B = ref.row_bound(x, y, metric)[live]
            assert np.isfinite(B).all() and (B * (1.0 - 2.0 ** -20) >= s).all(), (fam, name, float((B / s).min()))
            print("%s %s %s: B / summed bounds %.2f .. %.2f" % (shape, fam, name, (B / s).min(), (B / s).max()))


def test_the_device_bound_is_the_restated_one(built):
    """bound_of is compiled for the host as well (select_x3_bound: the same function refine_kernel evaluates): over every metric, widths
    32 .. 2048 and norms from 2^-13 to 2^5 on both sides its fp32 value agrees with the float64 restatement to 1e-5 - no term has a
    cancellation, so fp32 keeps about six digits - which is far inside the factor 1.25 the bound carries for it."""
    lib = ctypes.CDLL(LIB)
    lib.select_x3_bound.restype = ctypes.c_float
    lib.select_x3_bound.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 3
    worst = 0.0
    for name, metric in sorted(ref.METRICS.items()):
        for ld in (32, 64, 128, 512, 1280, 2048):
            for xx in (2.0 ** -26, 1e-3, 0.5, 1.0, 37.0, 1000.0):
                for ymax, ymin in ((1.0, 1.0), (1.0, 0.25), (900.0, 2.0 ** -20), (3e-4, 1e-4)):
                    got = lib.select_x3_bound(metric, ld, xx, ymax, ymin)
                    want = float(ref.bound_closed(metric, ld, np.float64(np.float32(xx)), float(np.float32(ymax)), float(np.float32(ymin))))
                    worst = max(worst, abs(got / want - 1.0))
                    assert abs(got / want - 1.0) < 1e-5, (name, ld, xx, ymax, ymin, got, want)
    print("largest relative difference between bound_of (fp32) and bound_closed (float64): %.2g" % worst)


# ---------------------------------------------------------------------------------------------- 5. Python rules without a device
class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_precision_and_k_are_checked_before_the_device(monkeypatch):
    x = np.zeros((2, 4), np.float32)
    import reid_amd.engine as engine_mod

    def no_engine(device=0):
        raise AssertionError("reached the device")
    monkeypatch.setattr(engine_mod, "get_engine", no_engine)
    monkeypatch.setattr(distance, "get_engine", no_engine)
    for bad in ("f16", 1, True, "", "F16X3", 2, ("f16x3",)):
        with pytest.raises(ValueError):
            Engine.argmin_rows(_NoDevice(), x, x, _ffi.METRIC_L2, precision=bad)
        with pytest.raises(ValueError):
            Engine.argmin_rows_dev(_NoDevice(), 0, 2, 0, 2, 4, _ffi.METRIC_L2, 0, precision=bad)
        with pytest.raises(ValueError):
            Engine.knn(_NoDevice(), x, x, 1, precision=bad)
        with pytest.raises(ValueError):
            Engine.knn_dev(_NoDevice(), 0, 2, 0, 2, 4, 1, 0, 0, precision=bad)
    for k in (0, 25, -1, 2.0, True):
        with pytest.raises(ValueError):
            Engine.knn(_NoDevice(), x, x, k, precision="f16x3")
        with pytest.raises(ValueError):
            Engine.knn_dev(_NoDevice(), 0, 2, 0, 2, 4, k, 0, 0, precision="f16x3")
        with pytest.raises(ValueError):
            distance.search_raw_array_x3(x, x, k)                                  # before the engine is made
    for k in (1, 24):
        with pytest.raises(AssertionError, match="reached the device"):
            distance.search_raw_array_x3(x, x, k)
    with pytest.raises(AssertionError, match="reached the device"):
        distance.nearest_x3(x, x)


def test_signatures():
    for fn in (distance.nearest, distance.search_raw_array, distance.IndexFlatL2.__init__, distance.IndexFlatL2.search):
        assert "precision" not in inspect.signature(fn).parameters, fn
    assert list(inspect.signature(distance.nearest).parameters) == ["x", "y", "metric", "device"]
    assert list(inspect.signature(distance.search_raw_array).parameters) == ["xb", "xq", "k", "device"]
    assert list(inspect.signature(distance.nearest_x3).parameters) == ["x", "y", "metric", "device"]
    assert list(inspect.signature(distance.search_raw_array_x3).parameters) == ["xb", "xq", "k", "device"]
    for fn in (Engine.argmin_rows, Engine.argmin_rows_dev, Engine.knn, Engine.knn_dev):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "precision" and p["precision"].default is None, fn


def test_which_entry_a_precision_reaches():
    """None and "f32" call today's entries, "f16x3" the new ones, with the same arguments."""
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
        Engine.argmin_rows(_Eng(), x, x, _ffi.METRIC_COS, precision=p)
        Engine.argmin_rows_dev(_Eng(), 0, 2, 0, 2, 4, _ffi.METRIC_COS, 0, precision=p)
        Engine.knn(_Eng(), x, x, 2, precision=p)
        Engine.knn_dev(_Eng(), 0, 2, 0, 2, 4, 2, 0, 0, precision=p)
    Engine.argmin_rows(_Eng(), x, x)
    Engine.knn(_Eng(), x, x, 30)                                                   # the exact entry keeps its own range of k
    exact = ["reid_argmin_rows", "reid_argmin_rows_dev", "reid_knn", "reid_knn_dev"]
    assert calls == exact * 2 + ["reid_argmin_rows_x3", "reid_argmin_rows_x3_dev", "reid_knn_x3", "reid_knn_x3_dev", "reid_argmin_rows", "reid_knn"]
