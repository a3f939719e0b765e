"""CPU checks of tests/postproc_ref.py, the reference side of tests/test_gpu_postproc.py: every de-biasing case lies in its condition-number
class and the yardstick's own error (fp32 LAPACK against float64) is as small as the bound assumes; the oracles agree with the fixture the
reference's own functions wrote (tests/golden/postproc.npz) and with oracle/postproc.py; the case tables reach what they claim to reach;
the harness entries are declared, bound and exported."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import matching, postproc
from reid_amd import _ffi
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postproc_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "postproc.npz"))


# ---------------------------------------------------------------------------------------------- de-biasing: the inputs of the GPU test
def _kappa_eref(case):
    x, la = ref.debias_case(case)
    want = ref.debias_cam64(x, la)
    assert np.isfinite(want).all()
    return ref.cond(x, la), float(np.abs(ref.debias_cam_ref32(x, la).astype(np.float64) - want).max())


@pytest.mark.parametrize("case", ref.DEBIAS_REQUIRED, ids=ref.case_id)
def test_required_case_is_in_its_class(case):
    kappa, e_ref = _kappa_eref(case)
    assert kappa <= ref.KAPPA_REQUIRED and e_ref <= ref.E_REF_REQUIRED, (kappa, e_ref)


@pytest.mark.parametrize("case", ref.DEBIAS_STIFF, ids=ref.case_id)
def test_stiff_case_is_in_its_class(case):
    kappa, e_ref = _kappa_eref(case)
    assert ref.KAPPA_REQUIRED < kappa <= ref.KAPPA_STIFF and e_ref <= ref.E_REF_STIFF, (kappa, e_ref)


def test_debias_case_table_keeps_what_it_must():
    """About 30 cases from the product of the issue's values, at least 8 stiff, every d and every rows-per-camera value in each class's
    union, no case twice; rows are `scale` long; the widths pad to 32, 132 and 260."""
    cases = ref.DEBIAS_REQUIRED + ref.DEBIAS_STIFF
    assert 28 <= len(cases) <= 36 and len(set(cases)) == len(cases) and len(ref.DEBIAS_STIFF) >= 8
    for table in (cases, ref.DEBIAS_STIFF):
        assert {c[0] for c in table} == set(ref.DEBIAS_D) and {c[1] for c in table} == set(ref.ROW_TAGS)
    assert {c[2] for c in cases} == {0.05, 5e-3, 5e-4} and {c[3] for c in cases} == {0.125, 1.0, 8.0}
    assert [(d + 3) // 4 * 4 for d in ref.DEBIAS_D] == [32, 132, 260]
    for case in cases:
        x, la = ref.debias_case(case)
        assert x.dtype == np.float32 and x.shape == (ref.rows_of(case[0], case[1]), case[0]) and la == case[2]
        np.testing.assert_allclose(np.linalg.norm(x.astype(np.float64), axis=1), case[3], rtol=1e-6)
    assert max(ref.rows_of(d, t) * d for d in ref.DEBIAS_D for t in ref.ROW_TAGS) == 771 * 257      # the largest problem


def test_debias_oracles_agree_with_the_reference_fixture(fx):
    """debias_ref32 (the reference's arithmetic), debias64 and oracle/postproc.py against what the reference's own function wrote."""
    want = fx["debiased"]
    for got in (ref.debias_ref32(fx["x"], fx["cams"]), ref.debias64(fx["x"], fx["cams"]), postproc.diminish_camera_bias(fx["x"], fx["cams"])):
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-5)
    # the two float64 restatements differ only in where the mean is subtracted (fp32 in oracle/postproc.py, as the reference; float64 here)
    np.testing.assert_allclose(ref.debias64(fx["x"], fx["cams"]), postproc.diminish_camera_bias(fx["x"], fx["cams"]), rtol=0, atol=1e-6)
    for c in np.unique(fx["cams"]):
        assert ref.cond(fx["x"][fx["cams"] == c], 0.05) <= ref.KAPPA_REQUIRED                        # what the suite pinned so far


def test_structure_case():
    """Five cameras {0, 2, 3, 7, 9} of 3d, 2, d, 1, d / 2 interleaved rows, every one in the required class; the single row is 0 / 0."""
    for d in (130, 257):
        x, cams, sizes = ref.struct_case(d)
        assert sizes == (3 * d, 2, d, 1, d // 2) and sorted(set(cams.tolist())) == list(ref.STRUCT_IDS)
        assert (np.diff(cams) != 0).mean() > 0.4                                                    # interleaved, not blocks
        want = ref.debias64(x, cams)
        for cid, m in zip(ref.STRUCT_IDS, sizes):
            sel = cams == cid
            assert sel.sum() == m
            assert np.isnan(want[sel]).all() if m == 1 else (np.isfinite(want[sel]).all() and ref.cond(x[sel], 0.05) <= ref.KAPPA_REQUIRED)


def test_two_step_oracle():
    """Two Newton-Schulz updates from I / ||A||_inf: the closed form X2 = sum_{k<4} (I - A / a)^k / a, far from the inverse at kappa >= 50."""
    assert ref.ITERS2_CASE in ref.DEBIAS_REQUIRED
    x, la = ref.debias_case(ref.ITERS2_CASE)
    assert ref.cond(x, la) >= 50
    cur = x.astype(np.float64)
    a = cur.T @ cur + len(cur) * la * np.eye(cur.shape[1])
    alpha = np.abs(a).sum(1).max()
    e = np.eye(len(a)) - a / alpha
    x2 = (np.eye(len(a)) + e + e @ e + e @ e @ e) / alpha
    cen = cur - cur.mean(0)
    y = cen @ x2
    np.testing.assert_allclose(ref.debias_two_steps64(x, la), y / np.linalg.norm(y, axis=1, keepdims=True), rtol=0, atol=1e-12)
    assert np.abs(ref.debias_two_steps64(x, la) - ref.debias_cam64(x, la)).max() > 1e-3


def test_host_entry_checks_the_ridge():
    """reid_cam_debias refuses la <= 0 (and NaN) before it queues anything, as reid_cam_debias_dev does."""
    src = open(os.path.join(CSRC, "postproc.hip")).read()
    for entry in ("reid_cam_debias_dev", "reid_cam_debias"):
        body = src.split('extern "C" int %s(' % entry)[1]
        first = body[body.index("{"):].split(";")[0]
        assert "ARG_CHECK" in first and "la > 0.f" in first, entry


# ---------------------------------------------------------------------------------------------- smoothing
def test_smooth_oracle_agrees_with_the_reference_fixture(fx):
    want, bound, count = ref.smooth64(fx["st_x"], fx["st_seq"], fx["st_valid"], 0.1)
    np.testing.assert_allclose(want, fx["st_out"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(want, postproc.smooth_tracklets(fx["st_x"], fx["st_seq"], fx["st_valid"]), rtol=0, atol=2e-6)
    assert (bound[~fx["st_valid"]] == 0).all() and (count[~fx["st_valid"]] == 0).all() and (bound[fx["st_valid"]] > 0).all()
    assert (np.abs(fx["st_out"] - want) <= 4 * bound + 1e-7)[fx["st_valid"]].all()          # torch sums in a tree: same order of size


@pytest.mark.parametrize("mask", ["none", "mixed", "allfalse"])
def test_smooth_cases_reach_what_they_claim(mask):
    for d in ref.SMOOTH_D:
        x, seqs, valid = ref.smooth_case(d, mask)
        assert x.shape == (1013, d) and seqs.dtype == np.int32
        assert {ref.INT32_MIN, ref.INT32_MAX, -5, -1}.issubset(set(seqs.tolist()))
        assert (np.diff(seqs.astype(np.int64)) < 0).any() and (np.diff(seqs.astype(np.int64)) != 0).mean() > 0.01   # unsorted, interleaved
        _, bound, count = ref.smooth64(x, seqs, valid, 0.5)
        if mask == "none":
            assert valid is None and sorted(np.unique(count).tolist()) == [1, 2, 7, 1000]
        elif mask == "mixed":
            assert 0 < valid.sum() < len(valid) and not valid[seqs == -1].any()              # one tracklet has no valid row at all
            assert (count[valid] >= 1).all() and (count[~valid] == 0).all() and (count == 1).any() and count.max() > 600
        else:
            assert not valid.any() and (bound == 0).all()
    assert [(d + 255) // 256 for d in ref.SMOOTH_D] == [1, 1, 1, 2, 3]                        # both sides of the 256-column slice


def test_smooth_oracle_properties():
    x, seqs, valid = ref.smooth_case(257, "mixed")
    out1, _, _ = ref.smooth64(x, seqs, valid, 1.0)
    assert np.array_equal(out1, x.astype(np.float64))
    out0, _, _ = ref.smooth64(x, seqs, valid, 0.0)
    for s in np.unique(seqs):
        rows = out0[(seqs == s) & valid]
        assert (rows == rows[:1]).all()
    # the mean divides by L: a tracklet of two rows a, b goes to their midpoint at keep = 0
    two = np.asarray([[1.0, 5.0], [3.0, -1.0]], np.float32)
    assert np.array_equal(ref.smooth64(two, [4, 4], None, 0.0)[0], [[2.0, 2.0], [2.0, 2.0]])


# ---------------------------------------------------------------------------------------------- descriptor, flip, DIoU
def test_descriptor_oracle_against_the_fp32_one():
    for (de, dl) in ref.DESC_DIMS:
        e1, l1, e2, l2 = ref.desc_inputs(de + dl, 5, de, dl)
        for a in (e1, l1, e2, l2):
            assert a.dtype == np.float32 and np.abs(a).min() >= 1e-3 and np.abs(a).max() <= 1e3
        one, two = ref.descriptor64(e1, l1), ref.tta_descriptor64(e1, l1, e2, l2)
        np.testing.assert_allclose(one, postproc.descriptor(e1, l1), rtol=0, atol=5e-7)
        np.testing.assert_allclose(two, postproc.tta_descriptor(e1, l1, e2, l2), rtol=0, atol=5e-7)
        np.testing.assert_allclose(np.linalg.norm(one[:, :de], axis=1), 1.0, atol=1e-14)    # two unit vectors, not renormalised
        np.testing.assert_allclose(np.linalg.norm(one, axis=1), np.sqrt(2.0), atol=1e-14)
        nrm = np.linalg.norm(two, axis=1)                                                   # 1 x 1: opposite signs in both halves average to the zero row
        assert ((np.abs(nrm - 1.0) <= 1e-14) | ((nrm == 0) & (de + dl == 2))).all() and (nrm > 0).any()
        assert 20 * ref.U < ref.desc_bound(de, dl) < 40 * ref.U
    assert abs(ref.desc_bound(512, 751) - 2e-6) < 2e-7
    z = np.zeros((1, 4), np.float32)
    assert (ref.descriptor64(z, z) == 0).all() and (ref.tta_descriptor64(z, z, z, z) == 0).all()   # the clamp, not 0 / 0


def test_flip_and_diou_tables():
    assert set(((1, 1), (5, 7), (3 * 256 * 2, 128), (3 * 256 * 8, 128))).issubset(ref.FLIP_SHAPES)
    assert ref.FLIP_SHAPES[-1][0] * ref.FLIP_SHAPES[-1][1] > 8192 * 256 >= ref.FLIP_SHAPES[-2][0] * ref.FLIP_SHAPES[-2][1]   # the grid cap
    assert ref.DIOU_SHAPES == ((1, 256), (1, 257), (3, 100), (40, 31))
    tracks, dets = ref.diou_boxes(40, 31)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = matching.diou(tracks[0], dets)
        cost = matching.diou_cost(tracks, dets)
    assert v[0] == 1.0                                                  # identical
    assert v[1] < 0 and v[3] < 0                                        # disjoint; edge-touching: IoU exactly 0
    inter3 = max(0.0, min(50.0, 75.0) - max(10.0, 50.0))
    assert inter3 == 0.0
    assert 0 < v[2] < 1                                                 # contained
    assert np.isfinite(v[4]) and np.isfinite(v[6]) and np.isfinite(v[7])   # zero width against a real box; 1e6 coordinates
    assert np.isnan(cost[5, 5]) and np.isnan(cost[4, 4])                # the all-zero pair and the zero-width pair: 0 / 0
    assert cost[0, 0] == 0.0 and cost[6, 6] == 0.0 and np.abs(dets[6:8]).max() >= 1e6


# ---------------------------------------------------------------------------------------------- the harness entries
def test_harness_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    internal = open(os.path.join(CSRC, "reid_internal.h")).read()
    src = open(os.path.join(CSRC, "postproc.hip")).read()
    for sym in ("reid_debug_descriptor", "reid_debug_flip_w"):
        assert "int %s(" % sym in hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), sym)
    assert hasattr(Engine, "debug_descriptor") and hasattr(Engine, "debug_flip_w")
    for fn in ("launch_descriptor", "launch_flip_w_nchw"):
        assert "int %s(" % fn in internal and "int %s(" % fn in src
    # the forward goes through the launchers: the kernels are launched nowhere else
    assert len(re.findall(r"hipLaunchKernelGGL\(descriptor_kernel", src)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(flip_w_nchw_kernel", src)) == 1
    assert len(re.findall(r"launch_descriptor\(ctx", src)) == 2 and len(re.findall(r"launch_flip_w_nchw\(ctx", src)) == 1
