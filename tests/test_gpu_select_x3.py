"""Arg-min and k-NN with fp32-class candidates on the MI355X (pytest -m gpu tests/test_gpu_select_x3.py): reid_argmin_rows_x3* and
reid_knn_x3* (csrc/select_x3.hip in libreid_hip_select_x3.so) are held to the EXACT entries reid_argmin_rows* / reid_knn* of the same
context, bit for bit - indices and values - and their proof to the float64 oracle of tests/distmat_x3_ref.py.
  1. bit equality on the shapes of tests/select_x3_ref.py, random operands (unit and not), five metrics, k in {1, 5, 24}, k > n, host and
     device entries;  2. on those sets no row is recomputed (every row's float64 gap between the k-th and the (k + 8)-th value exceeds 16
     times the summed bounds: a condition on the proof, not a timing);  3. exact duplicates in different column tiles (the lower column
     wins) and more 2^-20 near-ties than there are candidates (every such row is recomputed), forced fallbacks;  4. the exact family,
     and a gallery sorted by identity (tile lists that fill: no clear row is recomputed);
  5. a row's answer does not depend on the batch or its position, both tile forms;  6. the domain;  7. the exact entries keep their
     bits;  8. a build without the side library;  9. one Market-width case.
Every device output has a guard row preset to 0xff that must come back untouched."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi
from reid_amd._ffi import ReidHipError
from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distmat_x3_ref as x3  # noqa: E402
import select_x3_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu]
X3 = "f16x3"
GUARD = np.uint32(0xffffffff)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.clear_fault()
    yield e
    e.clear_fault()


def _dev(eng, x, y, metric, k, how="debug", force=0):
    """One launch on device operands into D, I [m + 1, k] preset to 0xff: how = "argmin" / "knn" - the _dev entry -, "debug" - the
    launcher through reid_debug_select_x3, with its statistics.  Returns (D bits [m, k], I [m, k], stats or None) after checking the
    guard row and that every output was written."""
    m, d = x.shape
    n = y.shape[0]
    dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
    dD = DevArray.from_numpy(eng, np.full((m + 1, k), GUARD, np.uint32))
    dI = DevArray.from_numpy(eng, np.full((m + 1, k), GUARD, np.uint32))
    stats = None
    try:
        if how == "argmin":
            assert k == 1
            eng.argmin_rows_dev(dx.ptr, m, dy.ptr, n, d, metric, dI.ptr, dD.ptr, precision=X3)
        elif how == "knn":
            eng.knn_dev(dx.ptr, m, dy.ptr, n, d, k, dD.ptr, dI.ptr, precision=X3)
        else:
            stats = eng.debug_select_x3(dx.ptr, m, dy.ptr, n, d, metric, k, dD.ptr, dI.ptr, force)
        eng.sync()
        D, I = dD.numpy(), dI.numpy()
    finally:
        for a in (dx, dy, dD, dI):
            a.free()
    assert (D[m] == GUARD).all() and (I[m] == GUARD).all(), "a guard row was written"
    I = I[:m].view(np.int32)
    assert (I >= -1).all() and (I < n).all(), "an index outside the gallery"
    assert eng.fault_bits() == 0
    return D[:m].copy(), I.copy(), stats


def _same(got_D, got_I, want_D, want_I, what):
    want_I = np.asarray(want_I).reshape(got_I.shape)
    assert np.array_equal(got_I, want_I), "%s: %d indices differ, first at %s" % (what, (got_I != want_I).sum(), np.argwhere(got_I != want_I)[0])
    want_D = _bits(want_D).reshape(got_D.shape)
    assert np.array_equal(got_D, want_D), "%s: %d values differ" % (what, (got_D != want_D).sum())


CASES = [(s, u) for s in ref.SHAPES for u in (False, True)]


# ---------------------------------------------------------------------------------------------- 1. + 2. the exact entries' bits, no row redone
@pytest.mark.parametrize("shape,unit", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_argmin_has_the_exact_entrys_bits_and_proves_every_row(eng, shape, unit):
    m, n, d = shape
    for name, metric in sorted(ref.METRICS.items()):
        x, y, clear, gap, b = ref.float64_case(shape, metric, unit, 1)
        assert clear.all(), "%s %s: %d rows of the reference are not clear" % (name, shape, (~clear).sum())
        idx, val = eng.argmin_rows(x, y, metric)
        D, I, stats = _dev(eng, x, y, metric, 1)
        _same(D, I, val, idx, "%s %s launcher" % (name, shape))
        print("%s %s unit %d: recomputed %d of %d, smallest float64 gap %.3g, largest summed bound %.3g" % (name, shape, unit, stats["recomputed"], m, gap, b.max()))
        assert stats["recomputed"] == 0 and stats["proven"] == m and stats["kk"] == ref.KK
        assert stats["form"] == (1 if n <= 64 else 2)
        D, I, _ = _dev(eng, x, y, metric, 1, "argmin")
        _same(D, I, val, idx, "%s %s device entry" % (name, shape))
        hidx, hval = eng.argmin_rows(x, y, metric, precision=X3)
        _same(_bits(hval)[:, None], hidx[:, None], val, idx, "%s %s host entry" % (name, shape))


@pytest.mark.parametrize("shape,unit", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_knn_has_the_exact_entrys_bits_and_proves_every_row(eng, shape, unit):
    m, n, d = shape
    for k in (1, 5, 24):
        x, y, clear, gap, b = ref.float64_case(shape, ref.METRIC_L2SQR, unit, k)
        want_D, want_I = eng.knn(x, y, k)
        if k > n:
            assert (want_I[:, n:] == -1).all() and np.isposinf(want_D[:, n:]).all() and (want_I[:, :n] >= 0).all()
        D, I, stats = _dev(eng, x, y, ref.METRIC_L2SQR, k)
        _same(D, I, want_D, want_I, "k %d %s launcher" % (k, shape))
        assert clear.all()
        print("k %d %s unit %d: recomputed %d of %d, smallest float64 gap %.3g" % (k, shape, unit, stats["recomputed"], m, gap))
        assert stats["recomputed"] == 0
        D, I, _ = _dev(eng, x, y, ref.METRIC_L2SQR, k, "knn")
        _same(D, I, want_D, want_I, "k %d %s device entry" % (k, shape))
        hD, hI = eng.knn(x, y, k, precision=X3)
        _same(_bits(hD), hI, want_D, want_I, "k %d %s host entry" % (k, shape))


# ---------------------------------------------------------------------------------------------- 3. adversarial rows
@pytest.mark.parametrize("name", sorted(ref.METRICS))
def test_duplicates_and_near_ties(eng, name):
    metric = ref.METRICS[name]
    x, y, near = ref.adversarial_operands(negate=name == "DOT")
    idx, val = eng.argmin_rows(x, y, metric)
    assert idx[0] == 10 and idx[1] == 37, "the exact entry: the lower of two equal columns"
    D, I, stats = _dev(eng, x, y, metric, 1)
    _same(D, I, val, idx, name)
    assert I[0, 0] == 10 and I[1, 0] == 37
    for r, cols in near.items():
        assert I[r, 0] in cols
    print("%s: recomputed %d of 6" % (name, stats["recomputed"]))
    rows = sorted(near)
    assert rows == [2, 3, 4, 5]
    # the near-tie rows as a batch of their own: every one of them is recomputed, none proven
    D, I, stats = _dev(eng, x[2:6], y, metric, 1)
    _same(D, I, val[2:6], idx[2:6], name + " near-tie rows")
    assert stats["recomputed"] == 4 and stats["proven"] == 0, "a row with more near-ties inside B than candidates was proven"
    if metric == ref.METRIC_L2SQR:
        for k in (5, 24):
            want_D, want_I = eng.knn(x, y, k)
            D, I, stats = _dev(eng, x, y, metric, k)
            _same(D, I, want_D, want_I, "k %d" % k)
            D, I, stats = _dev(eng, x[2:6], y, metric, k)
            _same(D, I, want_D[2:6], want_I[2:6], "k %d near-tie rows" % k)
            assert stats["recomputed"] == 4 and stats["proven"] == 0


@pytest.mark.parametrize("force", (1, 3))
def test_forced_fallback_has_the_same_bits(eng, force):
    x, y = x3.random_operands(200, 260, 160)
    for metric, k in ((ref.METRIC_COS, 1), (ref.METRIC_L2, 1), (ref.METRIC_L2SQR, 20)):
        D0, I0, s0 = _dev(eng, x, y, metric, k)
        assert s0["recomputed"] == 0
        D, I, s = _dev(eng, x, y, metric, k, force=force)
        _same(D, I, D0.view(np.float32), I0, "force %d" % force)
        assert s["recomputed"] == (200 + force - 1) // force and s["proven"] == 200 - s["recomputed"]
    want_D, want_I = eng.knn(x, y, 20)
    _same(D, I, want_D, want_I, "forced rows against the exact entry")


# ---------------------------------------------------------------------------------------------- 4. the exact family
@pytest.mark.parametrize("shape", ((127, 129, 96), (3, 300, 33)), ids=str)
def test_exact_family(eng, shape):
    """Approximate and exact dot products coincide; ties are real (integers plus multiples of 2^-13): whatever the proof decides, the
    answer is the exact entry's."""
    x, y = x3.exact_operands(*shape)
    for name, metric in sorted(ref.METRICS.items()):
        idx, val = eng.argmin_rows(x, y, metric)
        D, I, stats = _dev(eng, x, y, metric, 1)
        _same(D, I, val, idx, name)
        print("exact family %s %s: recomputed %d of %d" % (shape, name, stats["recomputed"], shape[0]))
    for k in (5, 24):
        want_D, want_I = eng.knn(x, y, k)
        D, I, stats = _dev(eng, x, y, ref.METRIC_L2SQR, k)
        _same(D, I, want_D, want_I, "k %d" % k)
        print("exact family %s k %d: recomputed %d of %d" % (shape, k, stats["recomputed"], shape[0]))


# ---------------------------------------------------------------------------------------------- 4b. a gallery sorted by identity
@pytest.mark.parametrize("per_id", (16, 48))
def test_gallery_sorted_by_identity(eng, per_id):
    """Consecutive images per identity: a query's near columns - its own identity's and those of identities that resemble it - are
    neighbours, and more of them than a tile list holds (C = 32) pass the filter inside one tile.  The list then keeps the tile's C
    smallest and bounds the rest by its last, so the proof does not depend on the gallery's order: every row's float64 gap is clear
    here, and no row may be recomputed."""
    x, y, who = ref.clustered_operands(per_id)
    for name, metric, k in (("COS", ref.METRIC_COS, 1), ("L2", ref.METRIC_L2, 1), ("L2SQR", ref.METRIC_L2SQR, 20)):
        if k == 1:
            idx, val = eng.argmin_rows(x, y, metric)
            want_D, want_I = val, idx
            assert (idx // per_id == who).all()
        else:
            want_D, want_I = eng.knn(x, y, k)
        D, I, stats = _dev(eng, x, y, metric, k)
        _same(D, I, want_D, want_I, "%d per identity, %s k %d" % (per_id, name, k))
        a = ref.approx_values(x, y, metric)
        full = max(int((a[i, t:t + 128] <= np.sort(a[i])[ref.KK - 1]).sum()) for i in range(len(x)) for t in range(0, a.shape[1], 128))
        s = np.sort(x3.oracle(x, y, metric)[0], axis=1)
        clear = s[:, k + 7] - s[:, k - 1] > 16 * ref.summed_bounds(x, y, metric).max(1)
        print("%d per identity, %s k %d: recomputed %d of %d rows; most of a row's 32 nearest in one tile: %d" % (per_id, name, k, stats["recomputed"], len(x), full))
        assert clear.all() and stats["recomputed"] == 0


# ---------------------------------------------------------------------------------------------- 5. independence
def test_a_row_does_not_depend_on_the_batch_and_both_forms_are_reached(eng):
    x, y = x3.random_operands(130, 260, 160)
    forms = set()
    for yy in (y, y[:64]):
        for metric, k in ((ref.METRIC_L2, 1), (ref.METRIC_COS_HALF, 1), (ref.METRIC_L2SQR, 20)):
            D, I, s = _dev(eng, x, yy, metric, k)
            forms.add(s["form"])
            assert s["form"] == (1 if len(yy) <= 64 else 2)
            D5, I5, _ = _dev(eng, x[60:65], yy, metric, k)
            assert np.array_equal(D5, D[60:65]) and np.array_equal(I5, I[60:65])
            for i in (0, 64, 129):
                D1, I1, _ = _dev(eng, x[i:i + 1], yy, metric, k)
                assert np.array_equal(D1[0], D[i]) and np.array_equal(I1[0], I[i]), (metric, k, i)
    assert forms == {1, 2}


# ---------------------------------------------------------------------------------------------- 6. the domain
@pytest.mark.parametrize("which,value", (("y", 40.0), ("x", 1e5)))
def test_an_operand_outside_the_domain(eng, which, value):
    x, y = (a.copy() for a in x3.random_operands(130, 70, 100))
    want = eng.argmin_rows(x, y, ref.METRIC_L2)
    wantk = eng.knn(x, y, 5)
    (x if which == "x" else y)[67, 41] = value
    try:
        for call in (lambda: eng.argmin_rows(x, y, ref.METRIC_L2, precision=X3), lambda: eng.knn(x, y, 5, precision=X3)):
            with pytest.raises(ReidHipError) as ei:
                call()
            assert ei.value.status == -3 and eng.fault_bits() & 1
            eng.clear_fault()
            assert eng.fault_bits() == 0
        x, y = x3.random_operands(130, 70, 100)
        got = eng.argmin_rows(x, y, ref.METRIC_L2, precision=X3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
        gotk = eng.knn(x, y, 5, precision=X3)
        assert np.array_equal(gotk[1], wantk[1]) and np.array_equal(_bits(gotk[0]), _bits(wantk[0]))
    finally:
        eng.clear_fault()


# ---------------------------------------------------------------------------------------------- 7. the exact entries are untouched
def test_the_exact_entries_keep_their_bits(eng):
    x, y = x3.random_operands(200, 260, 160)
    for metric in sorted(ref.METRICS.values()):
        before = eng.argmin_rows(x, y, metric)
        eng.argmin_rows(x, y, metric, precision=X3)
        for after in (eng.argmin_rows(x, y, metric), eng.argmin_rows(x, y, metric, precision=None), eng.argmin_rows(x, y, metric, precision="f32")):
            assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
    before = eng.knn(x, y, 20)
    eng.knn(x, y, 20, precision=X3)
    for after in (eng.knn(x, y, 20), eng.knn(x, y, 20, precision=None)):
        assert np.array_equal(before[1], after[1]) and np.array_equal(_bits(before[0]), _bits(after[0]))


def test_arguments(eng):
    import ctypes
    x, y = x3.random_operands(5, 3, 32)
    idx = np.full(5, 7, np.int32)
    D = np.full((5, 2), 7.0, np.float32)
    I = np.full((5, 2), 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    am, kn = eng.lib.reid_argmin_rows_x3, eng.lib.reid_knn_x3
    assert am(eng.h, p(x), 0, p(y), 3, 32, 0, p(idx), None) == 0 and am(eng.h, p(x), 5, p(y), 0, 32, 0, p(idx), None) == 0
    for metric in (-1, 5):
        assert am(eng.h, p(x), 5, p(y), 3, 32, metric, p(idx), None) == -1
    assert kn(eng.h, p(x), 0, p(y), 3, 32, 2, p(D), p(I)) == 0 and kn(eng.h, p(x), 5, p(y), 0, 32, 2, p(D), p(I)) == 0
    for k in (0, 25, -1):
        assert kn(eng.h, p(x), 5, p(y), 3, 32, k, p(D), p(I)) == -1
    assert (idx == 7).all() and (D == 7.0).all() and (I == 7).all()
    assert am(eng.h, p(x), 5, p(y), 3, 32, 0, p(idx), None) == 0              # val may be NULL
    assert np.array_equal(idx, eng.argmin_rows(x, y, 0)[0]) and eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 8. without the side library
_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
x = np.arange(12, dtype=np.float32).reshape(3, 4) / 7
before = eng.argmin_rows(x, x, _ffi.METRIC_L2), eng.knn(x, x, 2), eng.distmat(x, x, _ffi.METRIC_L2, precision="f16x3")
bad = 0
for call in (lambda: eng.argmin_rows(x, x, _ffi.METRIC_L2, precision="f16x3"), lambda: eng.knn(x, x, 2, precision="f16x3")):
    try:
        call()
        bad += 1
    except _ffi.ReidHipError as e:
        print("RAISED", e.status, e)
        bad += not (e.status == -3 and "libreid_hip_select_x3.so" in str(e) and eng.fault_bits() == 0)
after = eng.argmin_rows(x, x, _ffi.METRIC_L2), eng.knn(x, x, 2), eng.distmat(x, x, _ffi.METRIC_L2, precision="f16x3")
same = all(np.array_equal(np.asarray(a), np.asarray(b)) for p, q in zip(before[:2], after[:2]) for a, b in zip(p, q)) and np.array_equal(before[2], after[2])
sys.exit(0 if bad == 0 and same else 3)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_select_x3.so, loaded through REID_HIP_LIB in a fresh child process: both new entries are
    REID_ERR_STATE naming the file, and reid_argmin_rows, reid_knn and reid_distmat_x3 work before and after."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_select_x3.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("RAISED -3") == 2 and lib in r.stdout


# ---------------------------------------------------------------------------------------------- 9. Market width
def test_market_width(eng):
    """512 x 15913 x 512 unit rows: the exact entries take their fused kernels here (csrc/dist_select.hip)."""
    rng = np.random.default_rng(3)
    x = rng.normal(size=(512, 512)).astype(np.float32)
    y = rng.normal(size=(15913, 512)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    for metric in (ref.METRIC_COS, ref.METRIC_L2):
        idx, val = eng.argmin_rows(x, y, metric)
        D, I, s = _dev(eng, x, y, metric, 1)
        _same(D, I, val, idx, "arg-min metric %d" % metric)
        print("512 x 15913 x 512 arg-min metric %d: recomputed %.2f %% of the rows" % (metric, 100.0 * s["recomputed"] / 512))
    want_D, want_I = eng.knn(x, y, 20)
    D, I, s = _dev(eng, x, y, ref.METRIC_L2SQR, 20)
    _same(D, I, want_D, want_I, "k = 20")
    print("512 x 15913 x 512 k = 20: recomputed %.2f %% of the rows" % (100.0 * s["recomputed"] / 512))
