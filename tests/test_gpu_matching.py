"""The exact-fp32 matching entries on the MI355X (pytest -m gpu tests/test_gpu_matching.py): reid_distmat*, reid_argmin_rows*, reid_knn*,
reid_diou* against the float64 oracles of tests/matching_ref.py, every launch form at the smallest shape at which it can go wrong (the
tables there say which row reaches which form and why; tests/test_matching_host.py holds the predicates against the tables).
  1. exact family (integer features): DOT and L2SQR bit for bit, L2 within one ulp, the cosine forms within 8 * 2^-24, in every form;
  2. two forms that accept the same shape give identical bits;
  3. rounded family: every metric within the derived bound (d + 4) 2^-24 S of float64; the largest err / bound is printed;
  4. selection: (D, I) of reid_knn and the index of reid_argmin_rows equal the oracle's lexsort, fused and two-pass, ties to the lowest column;
  5. non-finite distances: the matrix has NaN and inf where the oracle has them, and a NaN is no candidate of any selection path;
  6. the device entries into guarded outputs, argument checks, DIoU beyond its fixture.
Every matrix goes through reid_distmat_dev into an [m + 1, n] output preset to a marked NaN: every element of rows 0 .. m - 1 must have been
written, the guard row and the floats in front of the output must not.  Launch forms are forced through Engine.debug_switch only (f32_conv,
f32_dist_bk16, select_two_pass), restored in a finally.  Largest observed err / bound: DESIGN, "matching tests"."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_ref as ref  # noqa: E402
from oracle import matching  # noqa: E402

pytestmark = [pytest.mark.gpu]
MARK = np.uint32(0x7fc0dead)                      # a NaN no arithmetic produces: "never written"
NAMES = sorted(ref.METRICS)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


@contextlib.contextmanager
def switches(eng, **kw):
    before = {k: eng.debug_switch(k) for k in kw}
    try:
        for k, v in kw.items():
            eng.debug_switch(k, v)
        yield
    finally:
        for k, v in before.items():
            eng.debug_switch(k, v)


def _distmat(eng, x, y, metric, x_off=0, out_off=0):
    """reid_distmat_dev on x [m, d], y [n, d] into an [m + 1, n] matrix of MARK, x moved x_off and the output out_off floats off their
    allocations: returns rows 0 .. m - 1 after checking that each element was written and nothing around them."""
    m, d = x.shape
    n = y.shape[0]
    dx = DevArray.from_numpy(eng, np.concatenate([np.zeros(x_off, np.float32), x.ravel()]))
    dy = DevArray.from_numpy(eng, y)
    do = DevArray.from_numpy(eng, np.full((m + 1) * n + out_off, MARK, np.uint32).view(np.float32))
    try:
        eng.distmat_dev(dx.ptr + 4 * x_off, m, dy.ptr, n, d, metric, do.ptr + 4 * out_off)
        eng.sync()
        flat = do.numpy().view(np.uint32)
    finally:
        for a in (dx, dy, do):
            a.free()
    assert (flat[:out_off] == MARK).all(), "floats in front of the output were written"
    out = flat[out_off:].reshape(m + 1, n)
    assert (out[m] == MARK).all(), "the guard row was written"
    assert (out[:m] != MARK).all(), "%d outputs were left unwritten" % (out[:m] == MARK).sum()
    return out[:m].view(np.float32).copy()


def _dist_id(row):
    m, n, d, x_off, out_off, f32_conv, bk16, form = row
    return "%s-%dx%dx%d" % (form, m, n, d) + ("-xoff%d" % x_off if x_off else "") + ("-outoff%d" % out_off if out_off else "") + \
        ("-f32_conv0" if not f32_conv else "")


# ---------------------------------------------------------------------------------------------- 1. exact family, every form
@pytest.mark.parametrize("row", ref.DIST_TABLE, ids=_dist_id)
def test_exact_family_in_every_launch_form(eng, row):
    m, n, d, x_off, out_off, f32_conv, bk16, form = row
    x, y = ref.exact_operands(m, n, d)
    with switches(eng, f32_conv=f32_conv, f32_dist_bk16=bk16):
        for name in NAMES:
            got = _distmat(eng, x, y, ref.METRICS[name], x_off, out_off)
            bad = ref.exact_mismatch(got, x, y, ref.METRICS[name])
            assert bad == 0, "%s %s: %d of %d elements outside the allowance" % (name, _dist_id(row), bad, got.size)


# ---------------------------------------------------------------------------------------------- 2. forms agree
@pytest.mark.parametrize("family", ("exact", "rounded"))
@pytest.mark.parametrize("shape", ((129, 193, 96), (129, 65, 2048), (129, 64, 96)), ids=str)
def test_forms_that_accept_the_same_shape_give_identical_bits(eng, shape, family):
    """K-tiles of 16 and of 32 (the 128-wide LDS-DMA tile), the LDS-DMA kernel and gemm_f32_kernel (f32_conv = 0), and - per element - the
    64-wide and the 128-wide tile (columns 0 .. 63 of a 65-wide call against the 64-wide call): every one runs an element's MFMAs in the
    same K order, so the matrices are identical, rounded operands included."""
    m, n, d = shape
    x, y = ref.exact_operands(m, n, d) if family == "exact" else ref.rounded_operands(m, n, d, 10.0)
    for name in NAMES:
        metric = ref.METRICS[name]
        with switches(eng, f32_conv=1, f32_dist_bk16=1):
            want = _bits(_distmat(eng, x, y, metric))
            if n > 64:
                narrow = _bits(_distmat(eng, x, y[:64], metric))
                assert ref.dist_form(m, 64, d) == ref.DMA64 and np.array_equal(narrow, want[:, :64]), name
        with switches(eng, f32_conv=1, f32_dist_bk16=0):
            assert np.array_equal(_bits(_distmat(eng, x, y, metric)), want), (name, "K-tiles of 32")
        with switches(eng, f32_conv=0):
            assert np.array_equal(_bits(_distmat(eng, x, y, metric)), want), (name, "gemm_f32_kernel")


@pytest.mark.parametrize("name", NAMES)
def test_host_entry_equals_device_entry(eng, name):
    x, y = ref.rounded_operands(129, 193, 96, 10.0)
    assert np.array_equal(_bits(eng.distmat(x, y, ref.METRICS[name])), _bits(_distmat(eng, x, y, ref.METRICS[name])))
    assert eng.distmat(x[:0], y, ref.METRICS[name]).shape == (0, 193)


# ---------------------------------------------------------------------------------------------- 3. rounded family
@pytest.mark.parametrize("offset", (0.0, 10.0))
@pytest.mark.parametrize("row", ref.ROUNDED_TABLE, ids=_dist_id)
def test_rounded_family_within_the_float64_bound(eng, row, offset):
    m, n, d, x_off, out_off, f32_conv, bk16, form = row
    x, y = ref.rounded_operands(m, n, d, offset)
    shares = {}
    with switches(eng, f32_conv=f32_conv, f32_dist_bk16=bk16):
        for name in NAMES:
            shares[name] = ref.rounded_share(_distmat(eng, x, y, ref.METRICS[name], x_off, out_off), x, y, ref.METRICS[name])
    print("%s offset %g: largest err / bound %s" % (_dist_id(row), offset, " ".join("%s %.3g" % kv for kv in sorted(shares.items()))))
    assert max(shares.values()) <= 1.0, shares


# ---------------------------------------------------------------------------------------------- 4. selection, exact family
def _select_cases():
    for m, n, d, k, identical, form in ref.SELECT_TABLE:
        yield pytest.param(m, n, d, k, identical, 0, id="%s-%dx%dx%d-k%d%s" % (form, m, n, d, k, "-identical" if identical else ""))
        if form in (ref.FUSED_ARGMIN, ref.FUSED_SELECT):
            yield pytest.param(m, n, d, k, identical, 1,
                               id="%s-%dx%dx%d-k%d%s-select_two_pass" % (ref.TWO_PASS_TOPK, m, n, d, k, "-identical" if identical else ""))


@pytest.mark.parametrize("m,n,d,k,identical,two_pass", list(_select_cases()))
def test_knn_equals_the_oracles_lexsort_bit_for_bit(eng, m, n, d, k, identical, two_pass):
    x, y = ref.exact_operands(m, n, d, identical)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    with switches(eng, select_two_pass=two_pass):
        D, I = eng.knn(x, y, k)
    assert np.array_equal(I, Iw), "first difference at %s" % (np.argwhere(I != Iw)[0],)
    assert np.array_equal(_bits(D), _bits(Dw))
    if identical:
        assert np.array_equal(I, np.tile(np.arange(k, dtype=np.int32), (m, 1)))
    if k > n:
        assert (I[:, n:] == -1).all() and np.isposinf(D[:, n:]).all()


def _argmin_cases():
    seen = set()
    for m, n, d, k, identical, _ in ref.SELECT_TABLE:
        if (m, n, d, identical) in seen:
            continue
        seen.add((m, n, d, identical))
        form = ref.select_form(m, n, d, 1, entry="argmin")
        yield pytest.param(m, n, d, identical, 0, id="%s-%dx%dx%d%s" % (form, m, n, d, "-identical" if identical else ""))
        if form == ref.FUSED_ARGMIN:
            yield pytest.param(m, n, d, identical, 1, id="%s-%dx%dx%d%s-select_two_pass" % (ref.TWO_PASS_ARGMIN, m, n, d, "-identical" if identical else ""))


@pytest.mark.parametrize("m,n,d,identical,two_pass", list(_argmin_cases()))
def test_argmin_rows_every_metric_against_the_oracle(eng, m, n, d, identical, two_pass):
    """idx is the oracle's winner (lowest column among equals) for DOT, L2SQR and L2, whose order the exact family fixes; under the cosine
    forms on the rows float64 decides by more than twice the allowance - at least nine in ten (tests/test_matching_host.py).  In the
    all-identical gallery every element of a row has the same bits, so column 0 wins under every metric.  val as in the matrix tests."""
    x, y = ref.exact_operands(m, n, d, identical)
    for name in NAMES:
        metric = ref.METRICS[name]
        want = ref.oracle(x, y, metric)
        iw, vw = ref.argmin_rule(want)
        with switches(eng, select_two_pass=two_pass):
            idx, val = eng.argmin_rows(x, y, metric)
        if identical:
            assert (idx == 0).all(), name
        elif name.startswith("COS"):
            decided = ref.decided_rows(x, y, metric)
            assert ref.enough_decided(decided) and np.array_equal(idx[decided], iw[decided]), name
        else:
            assert np.array_equal(idx, iw), name
        if metric in (ref.METRIC_DOT, ref.METRIC_L2SQR):
            assert np.array_equal(_bits(val), _bits(vw)), name
        elif metric == ref.METRIC_L2:
            assert (ref.ulp_distance(val, vw.astype(np.float32)) <= 1).all()
        else:
            assert (np.abs(val.astype(np.float64) - vw) <= ref.COS_EXACT_ALLOW).all(), name


def test_knn_when_one_thread_holds_the_whole_top_k_exact_family(eng):
    """topk_rows_kernel's exact fallback (a thread's four-key list runs dry) on integer operands: the oracle's order and bits."""
    xq, xb, near = ref.one_thread_operands()
    Dw, Iw = ref.select(ref.oracle(xq, xb, ref.METRIC_L2SQR), 10)
    assert set(Iw.ravel().tolist()) <= set(near.tolist())
    D, I = eng.knn(xq, xb, 10)
    assert np.array_equal(I, Iw) and np.array_equal(_bits(D), _bits(Dw))


# ---------------------------------------------------------------------------------------------- 5. non-finite distances
def _nonfinite_matrix(eng, x, y, name):
    """The device's matrix, held against the oracle: NaN and +-inf exactly where float64 has them, everything else within the rounded bound."""
    metric = ref.METRICS[name]
    got = _distmat(eng, x, y, metric)
    want = ref.oracle(x, y, metric)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN at %s only on one side" % (name, np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist())
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf].astype(np.float32)), name
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        if metric == ref.METRIC_L2:
            err = np.abs(got.astype(np.float64) ** 2 - np.maximum(ref.oracle(x, y, ref.METRIC_L2SQR), 1e-12))
        else:
            err = np.abs(got.astype(np.float64) - want)
        assert (err[fin] <= ref.bound(x, y, metric)[fin]).all(), name
    return got, want


@pytest.mark.parametrize("name", ("L2", "L2SQR", "COS", "DOT"))
@pytest.mark.parametrize("shape", ref.NONFINITE_SHAPES, ids=lambda s: "%s-%dx%dx%d" % ((("two_pass" if s[1] < 2048 else "fused"),) + s))
def test_nan_distances_are_no_candidates(eng, shape, name):
    """x[1] and y[2] carry a NaN (sign bit clear / set), x[m - 1] and y[n - 1] are zero (0 / 0 under COS), and under DOT y[4] and y[n - 2]
    carry +inf / -inf.  The matrix propagates them as numpy does (REID_METRIC_L2 included: the clamp keeps NaN); the arg-min and, for L2SQR,
    the k-NN at k = 1 and 5 are the rule of include/reid_hip.h applied to that matrix - a NaN of either sign is never selected, the all-NaN
    query row answers (-1, NaN) / (-1, +inf), -inf wins - and the fused and the two-pass path give the same bits."""
    m, n, d = shape
    metric = ref.METRICS[name]
    x, y = ref.nonfinite_operands(m, n, d, name == "DOT")
    got, want = _nonfinite_matrix(eng, x, y, name)
    assert np.isnan(got[1]).all() and np.isnan(got[:, 2]).all()
    iw, vw = ref.argmin_rule(got)
    assert iw[1] == -1 and (iw != 2).all()
    results = []
    for two_pass in (0, 1):
        with switches(eng, select_two_pass=two_pass):
            idx, val = eng.argmin_rows(x, y, metric)
            assert np.array_equal(idx, iw), (two_pass, np.argwhere(idx != iw)[:4].tolist(), idx[:4], iw[:4])
            assert np.array_equal(_bits(val)[iw >= 0], _bits(vw)[iw >= 0]) and np.isnan(val[iw < 0]).all(), two_pass
            res = [idx, np.nan_to_num(val, nan=-7.0)]
            if name == "L2SQR":
                for k in (1, 5):
                    D, I = eng.knn(x, y, k)
                    Dw, Iw = ref.select(got, k)
                    assert np.array_equal(I, Iw) and np.array_equal(_bits(D), _bits(Dw)), (two_pass, k)
                    assert (I[1] == -1).all() and np.isposinf(D[1]).all() and (I != 2).all()
                    res += [D, I]
            results.append(res)
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    if name == "DOT":                                    # -inf is an ordinary value, the smallest: its lowest column wins the row
        has = np.isneginf(got).any(1)
        assert np.isneginf(vw[has]).all() and np.array_equal(iw[has], np.isneginf(got).argmax(1)[has]) and (has.any() or m <= 3)
        assert np.isnan(got[m - 1, 4]) and np.isposinf(np.abs(got[0, 4])) and np.isposinf(np.abs(got[0, n - 2]))
    if name == "COS":
        assert iw[m - 1] == -1 and np.isnan(got[:, n - 1]).all()


def test_knn_pads_a_row_short_of_candidates(eng):
    """(2, 5, 32), k = 4: three gallery rows carry a NaN (both sign bits) - two candidates and two pads for query 0; query 1 carries one
    itself - four pads, and (-1, NaN) from the arg-min under every metric."""
    x, y = ref.nan_gallery_operands()
    got = _distmat(eng, x, y, ref.METRIC_L2SQR)
    Dw, Iw = ref.select(got, 4)
    assert sorted(Iw[0].tolist()) == [-1, -1, 1, 4] and (Iw[1] == -1).all()
    D, I = eng.knn(x, y, 4)
    assert np.array_equal(I, Iw) and np.array_equal(_bits(D), _bits(Dw)) and np.isposinf(D[0, 2:]).all()
    for name in NAMES:
        idx, val = eng.argmin_rows(x, y, ref.METRICS[name])
        assert idx[0] in (1, 4) and idx[1] == -1 and np.isnan(val[1]) and np.isfinite(val[0]), name


# ---------------------------------------------------------------------------------------------- 6. device entries, arguments, DIoU
@pytest.mark.parametrize("shape", ((3, 300, 32), (128, 2049, 64)), ids=lambda s: "%s-%dx%dx%d" % ((ref.select_form(*s, 5),) + s))
def test_device_entries_into_guarded_outputs(eng, shape):
    """reid_argmin_rows_dev with d_val NULL and reid_knn_dev (k = 5) into outputs with eight marked elements on either side."""
    m, n, d = shape
    k, g = 5, 8
    x, y = ref.exact_operands(m, n, d)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
    d_idx = DevArray.from_numpy(eng, np.full(m + 2 * g, -7, np.int32))
    d_D = DevArray.from_numpy(eng, np.full(m * k + 2 * g, MARK, np.uint32).view(np.float32))
    d_I = DevArray.from_numpy(eng, np.full(m * k + 2 * g, -7, np.int32))
    try:
        eng.argmin_rows_dev(dx.ptr, m, dy.ptr, n, d, ref.METRIC_L2SQR, d_idx.ptr + 4 * g, None)
        eng.knn_dev(dx.ptr, m, dy.ptr, n, d, k, d_D.ptr + 4 * g, d_I.ptr + 4 * g)
        eng.sync()
        idx, D, I = d_idx.numpy(), d_D.numpy().view(np.uint32), d_I.numpy()
    finally:
        for a in (dx, dy, d_idx, d_D, d_I):
            a.free()
    for a, mark in ((idx, -7), (D, MARK), (I, -7)):
        assert (a[:g] == mark).all() and (a[-g:] == mark).all(), "an element beside the output was written"
    assert np.array_equal(idx[g:-g], Iw[:, 0])
    assert np.array_equal(I[g:-g].reshape(m, k), Iw) and np.array_equal(D[g:-g].reshape(m, k), _bits(Dw))


def test_device_entries_refuse_bad_arguments(eng):
    x, y = ref.exact_operands(3, 300, 32)
    dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
    out = DevArray.from_numpy(eng, np.full(3 * 300, MARK, np.uint32).view(np.float32))
    d_I = DevArray.from_numpy(eng, np.full(3 * 300, -7, np.int32))
    P = ctypes.c_void_p
    lib, h = eng.lib, eng.h
    try:
        knn = lambda xq=dx.ptr, nq=3, xb=dy.ptr, nb=300, d=32, k=5, D=out.ptr, I=d_I.ptr: lib.reid_knn_dev(h, P(xq), nq, P(xb), nb, d, k, P(D), P(I))  # noqa: E731
        assert knn(d=0) == -1 and knn(xq=None) == -1 and knn(xb=None) == -1 and knn(k=0) == -1 and knn(nb=0) == -1
        assert knn(D=None) == -1 and knn(I=None) == -1 and knn(nq=-1) == -1 and knn(nq=0) == 0
        arg = lambda xq=dx.ptr, m=3, xb=dy.ptr, n=300, d=32, metric=0, I=d_I.ptr: lib.reid_argmin_rows_dev(h, P(xq), m, P(xb), n, d, metric, P(I), None)  # noqa: E731
        assert arg(d=0) == -1 and arg(xq=None) == -1 and arg(xb=None) == -1 and arg(n=0) == -1 and arg(I=None) == -1
        assert arg(metric=5) == -1 and arg(metric=-1) == -1 and arg(m=0) == 0
        dist = lambda xq=dx.ptr, m=3, xb=dy.ptr, n=300, d=32, metric=0, o=out.ptr: lib.reid_distmat_dev(h, P(xq), m, P(xb), n, d, metric, P(o))  # noqa: E731
        assert dist(d=0) == -1 and dist(xq=None) == -1 and dist(xb=None) == -1 and dist(o=None) == -1 and dist(metric=5) == -1
        assert dist(metric=-1) == -1 and dist(m=0) == 0 and dist(n=0) == 0
        eng.sync()
        assert (out.numpy().view(np.uint32) == MARK).all() and (d_I.numpy() == -7).all(), "a refused call wrote its output"
    finally:
        for a in (dx, dy, out, d_I):
            a.free()
    xh, yh = np.asarray(x), np.asarray(y)
    D, I = np.zeros((3, 5), np.float32), np.zeros((3, 5), np.int32)
    host = lambda d=32, k=5, nb=300: lib.reid_knn(h, xh.ctypes.data_as(P), 3, yh.ctypes.data_as(P), nb, d, k, D.ctypes.data_as(P), I.ctypes.data_as(P))  # noqa: E731
    assert host(d=0) == -1 and host(k=0) == -1 and host(nb=0) == -1


@pytest.mark.parametrize("case", sorted(ref.diou_cases()))
def test_diou_bit_for_bit_beyond_the_fixture(eng, case):
    """reid_diou_cost / reid_diou against oracle/matching.py (numpy float64, the reference's operation order): t m of 255, 256 and 257,
    negative coordinates, coordinates near 1e8, touching, nested, zero-width and identical zero-size boxes (NaN on both sides;
    assert_array_equal treats NaN as equal)."""
    tracks, dets = ref.diou_cases()[case]
    with np.errstate(all="ignore"):
        want = matching.diou_cost(tracks, dets)
        want_row = matching.diou(tracks[0], dets)
    got = eng.diou_cost(tracks, dets)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(eng.diou(tracks[0], dets), want_row)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if case == "touching_nested_zero":
        assert np.isnan(got[5, 6]) and got[0, 1] > 1.0 and got[0, 0] == 0.0
