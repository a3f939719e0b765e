"""The evaluation script's post-processing on the MI355X (pytest -m gpu), kernel by kernel against the float64 restatements of
tests/postproc_ref.py: camera de-biasing (reid_cam_debias: nine small kernels, the fp32 GEMMs of a Newton-Schulz inverse and its stopping
rule), tracklet smoothing (smooth_tracklets_kernel), the retrieval descriptor and the column mirror (descriptor_kernel and
flip_w_nchw_kernel through reid_debug_descriptor / reid_debug_flip_w, the launchers descriptor_dev calls) and DIoU (diou_kernel).  Bounds
and their derivations are in tests/postproc_ref.py; every test prints its figures before it asserts (profiles/postproc_gpu_tests.log)."""
import os
import sys

import numpy as np
import pytest

from reid_amd import _ffi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postproc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ----------------------------------------------------------------------------- 1. camera de-biasing, one camera per call
def _debias_one(eng, case, cls):
    x, la = ref.debias_case(case)
    want = ref.debias_cam64(x, la)
    e_ref = float(np.abs(ref.debias_cam_ref32(x, la).astype(np.float64) - want).max())
    got = eng.cam_debias(x, np.zeros(len(x), np.int32), la)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("\npostproc debias %-8s %-24s kappa %9.3g  e_ref %.2e  err %.2e  err / e_ref %7.2f  err / bound %5.2f" % (
        cls, ref.case_id(case), ref.cond(x, la), e_ref, err, err / e_ref, err / ref.debias_bound(e_ref)))
    assert err <= ref.debias_bound(e_ref)


@pytest.mark.parametrize("case", ref.DEBIAS_REQUIRED, ids=ref.case_id)
def test_debias_required_class(eng, case):
    """kappa <= 150: within 8 e_ref + 1e-6 of the float64 oracle, e_ref the error of the reference's own fp32 LAPACK arithmetic."""
    _debias_one(eng, case, "required")


@pytest.mark.parametrize("case", ref.DEBIAS_STIFF, ids=ref.case_id)
def test_debias_stiff_class(eng, case):
    """150 < kappa <= 3e4 (small la, rows of norm 8, cameras with far fewer rows than columns): the same bound."""
    _debias_one(eng, case, "stiff")


@pytest.mark.parametrize("d", [130, 257])
def test_debias_five_cameras_interleaved(eng, d):
    """Ids {0, 2, 3, 7, 9} (ids without rows are skipped), rows interleaved, sizes in id order 3d, 2, d, 1, d / 2 - large, small, large: a
    workspace whose padding is stale from the camera before shows here.  The single-row camera is NaN in exactly its row, as the
    oracle's (0 / 0); every other camera is within its bound; each camera alone gives the bits of the joint call."""
    x, cams, sizes = ref.struct_case(d)
    la = 0.05
    want = ref.debias64(x, cams, la)
    r32 = ref.debias_ref32(x, cams, la)
    got = eng.cam_debias(x, cams, la)
    single = cams == ref.STRUCT_IDS[sizes.index(1)]
    assert single.sum() == 1 and np.isnan(want[single]).all() and np.isfinite(want[~single]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for cid, m in zip(ref.STRUCT_IDS, sizes):
        sel = cams == cid
        assert sel.sum() == m
        alone = eng.cam_debias(x[sel], np.zeros(m, np.int32), la)
        assert np.array_equal(_bits(alone), _bits(got[sel])), "camera %d alone differs from the joint call" % cid
        if m == 1:
            continue
        assert ref.cond(x[sel], la) <= ref.KAPPA_REQUIRED
        e_ref = float(np.abs(r32[sel].astype(np.float64) - want[sel]).max())
        err = float(np.abs(got[sel].astype(np.float64) - want[sel]).max())
        print("\npostproc debias joint d %d camera %d (%d rows): e_ref %.2e  err %.2e  err / e_ref %.2f" % (d, cid, m, e_ref, err, err / e_ref))
        assert err <= ref.debias_bound(e_ref)


@pytest.mark.parametrize("d", [1, 3])
def test_debias_tiny_width(eng, d):
    """d = 1 and d = 3 (padded to 4 columns), 10 rows: rows of +-1 for d = 1."""
    x = ref.debias_rows(40 + d, 10, d)
    cams = np.zeros(10, np.int32)
    want = ref.debias64(x, cams, 0.05)
    e_ref = float(np.abs(ref.debias_ref32(x, cams, 0.05).astype(np.float64) - want).max())
    got = eng.cam_debias(x, cams, 0.05)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("\npostproc debias d %d: e_ref %.2e  err %.2e" % (d, e_ref, err))
    assert np.isfinite(got).all() and err <= ref.debias_bound(e_ref)


def test_debias_two_explicit_steps(eng):
    """iters = 2 on a case with kappa >= 50: exactly two Newton-Schulz updates from I / ||A||_inf, then projection and normalisation.  After
    two steps the iterate is a degree-3 polynomial in a matrix of norm <= 1 with no cancellation: 1e-5 against the float64 run of the same."""
    x, la = ref.debias_case(ref.ITERS2_CASE)
    assert ref.cond(x, la) >= 50
    want = ref.debias_two_steps64(x, la)
    got = eng.cam_debias(x, np.zeros(len(x), np.int32), la, iters=2)
    err = float(np.abs(got.astype(np.float64) - want).max())
    far = float(np.abs(want - ref.debias_cam64(x, la)).max())
    print("\npostproc debias iters = 2: err %.2e against two float64 steps; those are %.2e from the converged result" % (err, far))
    assert far > 1e-3                           # two steps are nowhere near the inverse: a run that iterated on would not pass
    assert err <= 1e-5


def test_debias_same_call_three_times(eng):
    """The stopping rule reads a residual: three identical calls give identical bits (required class, every width)."""
    same = True
    for case in (ref.DEBIAS_REQUIRED[1], ref.DEBIAS_REQUIRED[11], ref.DEBIAS_REQUIRED[18]):
        x, la = ref.debias_case(case)
        cams = np.zeros(len(x), np.int32)
        runs = [eng.cam_debias(x, cams, la) for _ in range(3)]
        eq = all(np.array_equal(_bits(runs[0]), _bits(r)) for r in runs[1:])
        print("\npostproc debias determinism %-24s three calls bit-identical: %s" % (ref.case_id(case), eq))
        same = same and eq
    assert same


@pytest.mark.parametrize("la", [0.0, -0.05, float("nan")])
def test_debias_refuses_a_ridge_that_is_not_positive(eng, la):
    x = ref.debias_rows(3, 6, 8)
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.cam_debias(x, np.zeros(6, np.int32), la)
    assert ei.value.status == -1                # REID_ERR_ARG


# ----------------------------------------------------------------------------- 2. tracklet smoothing
@pytest.mark.parametrize("mask", ["none", "mixed", "allfalse"])
@pytest.mark.parametrize("d", ref.SMOOTH_D)
def test_smooth_tracklets(eng, d, mask):
    """Tracklets of 1, 2, 7 and 1000 rows in one call, ids unsorted, interleaved, negative, INT32_MIN and INT32_MAX; widths around the
    256-column slice; every keep.  Per element within the sequential-sum bound; invalid rows bit-identical; keep = 1 the input bit for bit;
    keep = 0 all valid rows of a tracklet bit-identical to each other; a one-row tracklet within 2 u |x|."""
    x, seqs, valid = ref.smooth_case(d, mask)
    vmask = np.ones(len(seqs), bool) if valid is None else valid
    for keep in ref.SMOOTH_KEEP:
        want, bound, count = ref.smooth64(x, seqs, valid, keep)
        got = eng.smooth_tracklets(x, seqs, valid, keep)
        assert np.array_equal(_bits(got[~vmask]), _bits(x[~vmask]))
        err = np.abs(got.astype(np.float64) - want)
        touched = vmask
        worst = float((err[touched] / bound[touched]).max()) if touched.any() else 0.0
        print("\npostproc smooth d %d mask %s keep %g: max err / bound %.3f, max err %.2e" % (d, mask, keep, worst, float(err.max())))
        assert (err <= bound).all()
        if mask == "allfalse":
            assert np.array_equal(_bits(got), _bits(x))
            continue
        if keep == 1.0:
            assert np.array_equal(_bits(got), _bits(x))
        if keep == 0.0:
            for s in np.unique(seqs):
                rows = got[(seqs == s) & vmask]
                if len(rows):
                    assert (_bits(rows) == _bits(rows[:1])).all(), "keep = 0: rows of tracklet %d differ" % s
        one = vmask & (count == 1)
        assert one.any()
        assert (np.abs(got[one].astype(np.float64) - x[one]) <= 2.0 * ref.U * np.abs(x[one])).all()
    if mask == "none":
        assert sorted(np.unique(count).tolist()) == [1, 2, 7, 1000]


# ----------------------------------------------------------------------------- 3. descriptor_kernel
@pytest.mark.parametrize("n", ref.DESC_N)
@pytest.mark.parametrize("dims", ref.DESC_DIMS, ids=lambda t: "%dx%d" % t)
def test_descriptor_one_and_two_views(eng, dims, n):
    de, dl = dims
    d = de + dl
    bound = ref.desc_bound(de, dl)
    e1, l1, e2, l2 = ref.desc_inputs(de * 7 + dl + n, n, de, dl)
    got1, guard1 = eng.debug_descriptor(e1, l1)
    got2, guard2 = eng.debug_descriptor(e1, l1, e2, l2)
    for guard in (guard1, guard2):
        assert (guard.view(np.uint32) == 0xffffffff).all()               # the row behind the output is untouched
    err1 = float(np.abs(got1.astype(np.float64) - ref.descriptor64(e1, l1)).max())
    err2 = float(np.abs(got2.astype(np.float64) - ref.tta_descriptor64(e1, l1, e2, l2)).max())
    print("\npostproc descriptor %dx%d n %d: one view %.2e, two views %.2e, bound %.2e" % (de, dl, n, err1, err2, bound))
    assert err1 <= bound and err2 <= bound
    # one view: the concatenation of two unit vectors, NOT renormalised; two views: unit norm
    g1 = got1.astype(np.float64)
    assert (np.abs(np.linalg.norm(g1[:, :de], axis=1) - 1.0) <= bound).all()
    assert (np.abs(np.linalg.norm(g1[:, de:], axis=1) - 1.0) <= bound).all()
    nz = np.linalg.norm(ref.tta_descriptor64(e1, l1, e2, l2), axis=1) > 0.5          # 1 x 1: views of opposite signs average to the zero row
    assert (np.abs(np.linalg.norm(got2.astype(np.float64), axis=1)[nz] - 1.0) <= bound).all() and (got2[~nz] == 0).all()
    assert d == got1.shape[1] == got2.shape[1]


@pytest.mark.parametrize("dims", ref.DESC_DIMS, ids=lambda t: "%dx%d" % t)
def test_descriptor_zero_rows(eng, dims):
    """F.normalize's clamp max(||x||, 1e-12): a row whose embedding is all zero gives zeros there, not NaN; a row where both views are
    all zero gives a zero final row."""
    de, dl = dims
    bound = ref.desc_bound(de, dl)
    e1, l1, e2, l2 = ref.desc_inputs(de * 11 + dl, 5, de, dl)
    e1[1] = 0.0                                 # row 1: the plain view's embedding is zero
    for a in (e1, l1, e2, l2):
        a[3] = 0.0                              # row 3: everything is zero
    got1, _ = eng.debug_descriptor(e1, l1)
    got2, _ = eng.debug_descriptor(e1, l1, e2, l2)
    assert np.isfinite(got1).all() and np.isfinite(got2).all()
    assert (got1[1, :de] == 0).all() and (got1[3] == 0).all() and (got2[3] == 0).all()
    assert np.abs(got1.astype(np.float64) - ref.descriptor64(e1, l1)).max() <= bound
    assert np.abs(got2.astype(np.float64) - ref.tta_descriptor64(e1, l1, e2, l2)).max() <= bound


# ----------------------------------------------------------------------------- 4. flip_w_nchw_kernel
@pytest.mark.parametrize("shape", ref.FLIP_SHAPES, ids=lambda t: "%dx%d" % t)
def test_flip_w(eng, shape):
    """Bit-identical to x[:, ::-1]; (16896, 128) has more than 8192 * 256 elements, so the grid-stride loop runs."""
    rows, w = shape
    x = np.random.default_rng(rows + w).standard_normal((rows, w)).astype(F)
    got, guard = eng.debug_flip_w(x)
    assert (guard.view(np.uint32) == 0xffffffff).all()
    assert np.array_equal(_bits(got), _bits(x[:, ::-1]))
    if w > 1:
        assert not np.array_equal(got, x)


# ----------------------------------------------------------------------------- 5. diou_kernel
@pytest.mark.parametrize("shape", ref.DIOU_SHAPES, ids=lambda t: "%dx%d" % t)
def test_diou_bit_for_bit(eng, shape):
    """Against oracle/matching.py (float64, the reference's operation order) bit for bit, NaN where the oracle is NaN: identical,
    disjoint, contained, edge-touching and zero-width boxes, the all-zero pair, coordinates of 1e6."""
    from oracle import matching
    t, m = shape
    tracks, dets = ref.diou_boxes(t, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_cost = matching.diou_cost(tracks, dets)
        want0 = matching.diou(tracks[0], dets)
    got_cost = eng.diou_cost(tracks, dets)
    got0 = eng.diou(tracks[0], dets)
    assert want0[0] == 1.0 and want0[3] < 0 and np.isnan(want0[5]) == np.isnan(got0[5])        # identical; touching: IoU 0; the zero box
    if t > 5:
        assert np.isnan(want_cost[5, 5])                                                     # the all-zero pair
    np.testing.assert_array_equal(got_cost, want_cost)                                       # NaN == NaN in this comparison
    np.testing.assert_array_equal(got0, want0)
    fin = np.isfinite(want_cost)
    assert np.array_equal(got_cost[fin].view(np.uint64), want_cost[fin].view(np.uint64))
