"""Host side of the Swin frame pipeline (no GPU): the new entry points' declarations and exports, the 96-wide cost kernel's library
(kernel list, scratch, independence), the stream classes' surface up to the first device call, and the helper tests/bank_ref.py - held
to oracle/nn_matching.py, with a numpy restatement of the kernel's 16-lane butterfly."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nn_matching as onm
from reid_amd import _ffi
from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream, ShardedCameraStream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_bank96.so")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_the_new_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert "reid_frame_submit_swin(" in hdr and "reid_frame_submit_swin" in _ffi.EXPORTS and hasattr(lib, "reid_frame_submit_swin")
    assert len(_ffi._SIGS["reid_frame_submit_swin"][1]) == 9
    dbg = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    assert "reid_debug_bank_cost96(" in dbg and "reid_debug_bank_cost96" in _ffi.DEBUG_EXPORTS
    assert hasattr(_ffi.debug_lib(), "reid_debug_bank_cost96")


def test_bank96_library_kernels_match_their_list(built, golden_dir):
    """bank_cost96_kernel lives in a library of its own, libreid_hip_bank96.so, that libreid_hip.so opens from its own directory on the
    first reid_frame_submit_swin: its kernel list equals tests/golden/kernels_bank96.json by name, the kernel has no scratch, the product
    library does not name it among what it needs, and it loads on its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_bank96.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 1 and "bank_cost96_kernel" in list(got)[0]
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_bank96" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own                            # ... and it needs nothing of the product library
    assert hasattr(ctypes.CDLL(LIB), "bank96_cost")


def test_stream_classes_take_arch_size_and_mean_std():
    """arch="swin" is part of the three stream classes' signatures (default: the ResNet path), and a size that is no multiple of 224
    raises ValueError before any device call - with no GPU in this test, anything that reached the engine would fail differently."""
    for cls, extra in ((CameraStream, ()), (MultiCameraStream, (2,)), (LookaheadCameraStream, ())):
        p = inspect.signature(cls.__init__).parameters
        assert p["arch"].default == "seres18" and p["size"].default == (224, 224) and p["mean_std"].default is None, cls
        with pytest.raises(ValueError, match="224"):
            cls(np.zeros(4, np.float32), "", *extra, arch="swin", size=(200, 224))
        with pytest.raises(ValueError):
            cls(np.zeros(4, np.float32), "", *extra, arch="swin", mean_std=[0.5, 0.5, 0.5, 0.2, 0.0, 0.2])
        with pytest.raises(ValueError, match="arch"):
            cls(np.zeros(4, np.float32), "", *extra, arch="osnet")
        assert callable(getattr(cls, "_submit"))
    assert "arch" not in inspect.signature(ShardedCameraStream.__init__).parameters and "Swin" in ShardedCameraStream.__doc__


def test_bank_ref_restates_the_oracle_metric():
    """bank_ref.RefBank and oracle/nn_matching.py (fed float64) agree on one case with truncation past the budget and both metrics."""
    assert (br.COS, br.L2) == (_ffi.METRIC_COS, _ffi.METRIC_L2SQR)
    rng = np.random.default_rng(0)
    feats = rng.normal(0, 1, (23, 96))
    keys = [0, 1, 2, 1, 1, 0, 2, 2, 2, 2, 1, 0, 1, 1, 1, 2, 0, 0, 0, 0, 1, 2, 1]
    dets = rng.normal(0, 1, (9, 96))
    for metric, name in ((br.COS, "cosine"), (br.L2, "euclidean")):
        ref = br.RefBank(5)
        orc = onm.NearestNeighborDistanceMetric(name, 0.2, 5)
        ref.partial_fit(feats, keys, [0, 1, 2])
        orc.partial_fit(list(feats), keys, [0, 1, 2])
        assert [ref.count(k) for k in (0, 1, 2)] == [5, 5, 5] and keys.count(1) > 5
        want = orc.distance(dets, [2, 0, 1])
        np.testing.assert_allclose(ref.cost([2, 0, 1], dets, metric), want, rtol=0, atol=1e-12)
        thr = float(np.sort(want.ravel())[13:15].mean())      # between two entries: both sides decide alike
        np.testing.assert_allclose(ref.cost([2, 0, 1], dets, metric, thr), onm.gate(want, thr), rtol=0, atol=1e-12)
        with pytest.raises(KeyError):
            orc.distance(dets, [7])
        with pytest.raises(KeyError):
            ref.cost([7], dets, metric)
        tol = ref.bound([2, 0, 1], dets, metric, br.CHAIN_96)
        assert tol.shape == want.shape and (tol > 0).all()
    assert br.CHAIN_96 == 10 and br.chain_generic(96) == 10 and br.chain_generic(512) == 16
    assert br.RefBank(3).bound([0], dets[:2], br.COS, br.CHAIN_96)[0, 0] == 2.0 * 26 * 2.0 ** -24


def test_butterfly_restatement_says_which_detection_a_lane_ends_with():
    """Lane l of a 16-lane group ends with the sum over the group of detection j(l) = its bits reversed, and nothing else; with two
    levels of the butterfly swapped that no longer holds."""
    rng = np.random.default_rng(3)
    v = rng.integers(-1000, 1000, (16, 16)).astype(np.float64)      # integers: every order of the additions gives the same sum
    j = br.lane_detection(np.arange(16))
    assert sorted(j.tolist()) == list(range(16)) and j[1] == 8 and j[2] == 4 and j[8] == 1 and j[15] == 15
    np.testing.assert_array_equal(br.butterfly_group(v), v.sum(0)[j])
    for swapped in ((1, 0, 2, 3), (0, 1, 3, 2), (3, 1, 2, 0)):
        assert not np.array_equal(br.butterfly_group(v, swapped), v.sum(0)[j]), swapped
    # one-hot inputs: lane l's result picks up partial sums of detection j(l) only, from all 16 lanes
    for lane in (0, 5, 10):
        for det in (0, 7, 12):
            e = np.zeros((16, 16))
            e[lane, det] = 1.0
            r = br.butterfly_group(e)
            assert r.sum() == 1.0 and r[np.flatnonzero(j == det)[0]] == 1.0
