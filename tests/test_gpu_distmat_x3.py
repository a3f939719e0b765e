"""The fp32-class distance matrix on the MI355X (pytest -m gpu tests/test_gpu_distmat_x3.py): reid_distmat_x3* and dist_x3_kernel of
libreid_hip_distmat_x3.so on the shapes of tests/distmat_x3_ref.py - the smallest at which each code path can go wrong.
  1. exact family, DOT: the output equals the numpy restatement's fp32 value BIT FOR BIT (tests/test_distmat_x3_host.py shows why fp32
     accumulation is exact there and which mutations it excludes);
  2. random operands with rows of y equal, and equal up to 2^-10, to rows of x: every metric within the bound derived in
     tests/distmat_x3_ref.py's docstring of the float64 oracle (L2 on its square);
  3. the small family (f16 subnormals in both parts of x) within the same bound;
  4. an element's bits do not depend on m, n or its position; 5. the exact entry keeps its bits around a call of the new one, and the two
     differ by no more than both bounds; 6. the range guard; 7. arguments, the two tile forms, a build without the side library;
  8. the arg-min agrees with the exact entry's on every row with a clear float64 winner.
Every launch goes through the device entry into a matrix with a guard row that must still read as NaN afterwards.
Largest observed err / bound on the MI355X (printed by every test): see DESIGN, "fp32-class distance matrix"."""
import ctypes
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
import distmat_x3_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu]
X3 = "f16x3"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.clear_fault()
    yield e
    e.clear_fault()


def _run(eng, x, y, metric, precision=X3, x_off=0, out_off=0):
    """The device entry on x [m, d], y [n, d] into an [m + 1, n] matrix of NaN: returns rows 0 .. m - 1, after checking that every one
    of them was written and that the guard row was not.  x_off / out_off: floats by which the operand / the output is moved off its
    allocation's alignment."""
    m, d = x.shape
    n = y.shape[0]
    dx = DevArray.from_numpy(eng, np.concatenate([np.zeros(x_off, np.float32), x.ravel()]))
    dy = DevArray.from_numpy(eng, y)
    do = DevArray.from_numpy(eng, np.full((m + 1) * n + out_off, np.nan, np.float32))
    try:
        eng.distmat_dev(dx.ptr + 4 * x_off, m, dy.ptr, n, d, metric, do.ptr + 4 * out_off, precision=precision)
        eng.sync()
        flat = do.numpy()
    finally:
        for a in (dx, dy, do):
            a.free()
    assert np.isnan(flat[:out_off]).all(), "floats in front of the output were written"
    out = flat[out_off:].reshape(m + 1, n)
    assert np.isnan(out[m]).all(), "the guard row was written"
    assert not np.isnan(out[:m]).any(), "an output was left unwritten (or is NaN)"
    assert eng.fault_bits() == 0
    return out[:m].copy()


def _held(got, x, y, metric, what, e_dot=None):
    share, ok = ref.check(got, x, y, metric, e_dot)
    print("%s: largest err / bound %.3g" % (what, share))
    assert ok, "%s: err / bound %.3g" % (what, share)
    return share


# ---------------------------------------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_exact_family_bit_for_bit(eng, shape):
    x, y = ref.exact_operands(*shape)
    val, mag = ref.restate(x, y)
    assert mag.max() / 0.25 < 2.0 ** 24
    got = _run(eng, x, y, _ffi.METRIC_DOT)
    want = val.astype(np.float32)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s" % (shape, diff.sum(), diff.size, np.argwhere(diff)[0])
    assert np.array_equal(_bits(eng.distmat(x, y, _ffi.METRIC_DOT, precision=X3)), _bits(want)), "the host entry"


# ---------------------------------------------------------------------------------------------- 2. float64 bound, every metric
@pytest.mark.parametrize("name", sorted(ref.METRICS))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_every_metric_within_the_float64_bound(eng, shape, name):
    metric = ref.METRICS[name]
    x, y = ref.random_operands(*shape, unit=name.startswith("COS"))
    got = _run(eng, x, y, metric)
    _held(got, x, y, metric, "%s %s" % (name, shape))


def test_descriptor_width_and_unaligned_buffers(eng):
    """d = 1263 (the descriptor: 40 K steps, a padded copy) on unit rows, and d = 64 with x four bytes off its alignment (the padded copy
    although d % 32 == 0) and the output four bytes off (n % 4 == 0, yet stores per element): the same bits as the aligned call."""
    x, y = ref.random_operands(9, 12, 1263, unit=True)
    for name in ("COS", "L2"):
        _held(_run(eng, x, y, ref.METRICS[name]), x, y, ref.METRICS[name], "%s (9, 12, 1263)" % name)
    x, y = ref.random_operands(40, 68, 64)
    want = _run(eng, x, y, _ffi.METRIC_L2SQR)
    assert np.array_equal(_bits(_run(eng, x, y, _ffi.METRIC_L2SQR, x_off=1)), _bits(want))
    assert np.array_equal(_bits(_run(eng, x, y, _ffi.METRIC_L2SQR, out_off=1)), _bits(want))


# ---------------------------------------------------------------------------------------------- 3. small family
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_small_family_keeps_f16_subnormals(eng, shape):
    x, y = ref.small_operands(*shape)
    _held(_run(eng, x, y, _ffi.METRIC_DOT), x, y, _ffi.METRIC_DOT, "small family %s" % (shape,))


# ---------------------------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("name", ("DOT", "L2", "COS"))
def test_an_element_does_not_depend_on_the_call(eng, name):
    """out[i][j] of the full call equals, bit for bit, the m = 1 call on row i, a call on a column subset containing j (three columns: the
    other tile form; 51 columns from 130 on: another tile, another offset in it, n % 4 != 0) and a call with rows and columns permuted."""
    metric = ref.METRICS[name]
    m, n, d = 200, 260, 160
    x, y = ref.random_operands(m, n, d, unit=name == "COS")
    full = _bits(_run(eng, x, y, metric))
    for i in (0, 77, 129, 199):
        assert np.array_equal(_bits(_run(eng, x[i:i + 1], y, metric))[0], full[i]), i
    for lo, hi in ((0, 3), (130, 181), (257, 260)):
        assert np.array_equal(_bits(_run(eng, x, y[lo:hi], metric)), full[:, lo:hi]), (lo, hi)
    rng = np.random.default_rng(5)
    pr, pc = rng.permutation(m), rng.permutation(n)
    assert np.array_equal(_bits(_run(eng, x[pr], y[pc], metric)), full[pr][:, pc])
    assert len(np.unique(full)) > full.size // 2


# ---------------------------------------------------------------------------------------------- 5. the exact entry is untouched
@pytest.mark.parametrize("name", sorted(ref.METRICS))
def test_exact_entry_keeps_its_bits_and_both_agree_within_their_bounds(eng, name):
    metric = ref.METRICS[name]
    x, y = ref.random_operands(200, 260, 160, unit=name.startswith("COS"))
    before = eng.distmat(x, y, metric)
    new = eng.distmat(x, y, metric, precision=X3)
    after = eng.distmat(x, y, metric)
    assert np.array_equal(_bits(before), _bits(after)) and np.array_equal(_bits(before), _bits(eng.distmat(x, y, metric, precision="f32")))
    assert not np.array_equal(_bits(before), _bits(new)), "the fp32-class entry returned the exact entry's bits"
    e_exact = ref.dot_bounds(x, y)[3]
    _held(before, x, y, metric, name + " exact entry", e_dot=e_exact)
    _held(new, x, y, metric, name + " fp32-class entry")
    want, b3 = ref.oracle(x, y, metric)
    b0 = ref.oracle(x, y, metric, e_exact)[1]
    a, b = new.astype(np.float64), before.astype(np.float64)
    if name == "L2":                                      # the bounds live on the square: |a - b| (a + b) = |a^2 - b^2|
        a, b = a * a, b * b
    assert (np.abs(a - b) <= b3 + b0).all()


# ---------------------------------------------------------------------------------------------- 6. the range guard
@pytest.mark.parametrize("which,value", (("y", 40.0), ("x", 1e5), ("x", np.nan), ("y", np.nan)))
def test_an_operand_outside_the_domain_raises_the_sticky_word(eng, which, value):
    x, y = (a.copy() for a in ref.random_operands(130, 70, 100))
    good = eng.distmat(x, y, _ffi.METRIC_L2, precision=X3)
    exact = eng.distmat(x, y, _ffi.METRIC_L2)
    (x if which == "x" else y)[67, 41] = value
    try:
        with pytest.raises(ReidHipError, match="outside f16's range") as ei:
            eng.distmat(x, y, _ffi.METRIC_L2, precision=X3)
        assert ei.value.status == -3 and eng.fault_bits() & 1
        with pytest.raises(ReidHipError) as ei:                             # sticky
            eng.distmat(*ref.random_operands(130, 70, 100), _ffi.METRIC_L2, precision=X3)
        assert ei.value.status == -3 and eng.fault_bits() & 1
        eng.clear_fault()
        assert eng.fault_bits() == 0
        x, y = ref.random_operands(130, 70, 100)
        assert np.array_equal(_bits(eng.distmat(x, y, _ffi.METRIC_L2, precision=X3)), _bits(good))
        assert np.array_equal(_bits(eng.distmat(x, y, _ffi.METRIC_L2)), _bits(exact))
    finally:
        eng.clear_fault()


def test_the_domain_edges_and_the_device_entry(eng):
    """|y| = 31.98 (just inside 65504 / 2^11) and |x| = 65000 pass; through the asynchronous device entry a bad operand is reported by
    the next synchronising call."""
    x, y = (a.copy() for a in ref.random_operands(5, 3, 32))
    y[1, 7], x[2, 9] = 31.98, -65000.0
    _held(_run(eng, x, y, _ffi.METRIC_DOT), x, y, _ffi.METRIC_DOT, "domain edges")
    y[1, 7] = 31.99
    dx, dy, do = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y), DevArray(eng, (5, 3))
    try:
        eng.distmat_dev(dx.ptr, 5, dy.ptr, 3, 32, _ffi.METRIC_DOT, do.ptr, precision=X3)
        with pytest.raises(ReidHipError) as ei:
            eng.sync()
        assert ei.value.status == -3 and eng.fault_bits() & 1
    finally:
        eng.clear_fault()
        for a in (dx, dy, do):
            a.free()
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 7. arguments, tile forms, missing library
def test_arguments(eng):
    x, y = ref.random_operands(5, 3, 32)
    out = np.full((5, 3), 7.0, np.float32)

    def call(m, n, d, metric, fn="reid_distmat_x3"):
        return getattr(eng.lib, fn)(eng.h, x.ctypes.data_as(ctypes.c_void_p), m, y.ctypes.data_as(ctypes.c_void_p), n, d, metric,
                                    out.ctypes.data_as(ctypes.c_void_p))
    assert call(0, 3, 32, 0) == 0 and call(5, 0, 32, 0) == 0 and (out == 7.0).all()
    for metric in (-1, 5, 99):
        assert call(5, 3, 32, metric) == -1 and (out == 7.0).all()
        assert call(5, 3, 32, metric, "reid_distmat") == -1
    assert call(5, 3, 0, 0) == -1 and call(-1, 3, 32, 0) == -1
    dx, dy, do = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y), DevArray(eng, (5, 3))
    try:
        dev = eng.lib.reid_distmat_x3_dev
        args = lambda m, n, metric: (eng.h, ctypes.c_void_p(dx.ptr), m, ctypes.c_void_p(dy.ptr), n, 32, metric, ctypes.c_void_p(do.ptr))  # noqa: E731
        assert dev(*args(0, 3, 0)) == 0 and dev(*args(5, 0, 0)) == 0 and dev(*args(5, 3, 5)) == -1 and dev(*args(5, 3, -1)) == -1
        assert dev(eng.h, None, 5, ctypes.c_void_p(dy.ptr), 3, 32, 0, ctypes.c_void_p(do.ptr)) == -1
    finally:
        for a in (dx, dy, do):
            a.free()
    # d = 1: a whole K step of which one column is real
    x1, y1 = ref.random_operands(1, 1, 1)
    for name, metric in sorted(ref.METRICS.items()):
        _held(_run(eng, x1, y1, metric), x1, y1, metric, name + " d = 1")
    assert eng.fault_bits() == 0


def test_every_tile_form_is_reached(eng):
    """distmat_x3 of the side library, called as api.hip calls it, reports the tile form it launched: a rule of n alone, and an element's
    bits are the same under both (the entry's result on the same operands)."""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(_ffi.LIB_PATH), "libreid_hip_distmat_x3.so"))
    lib.distmat_x3.restype = ctypes.c_int
    lib.distmat_x3.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    seen = set()
    for m, n, d in ((40, 64, 64), (40, 68, 64), (1, 1, 32), (130, 65, 32)):
        x, y = ref.random_operands(m, n, d)
        want = _run(eng, x, y, _ffi.METRIC_DOT)
        dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
        do = DevArray.from_numpy(eng, np.full((m + 1, n), np.nan, np.float32))
        form = ctypes.c_int(0)
        try:
            eng.device_sync()
            assert lib.distmat_x3(None, dx.ptr, m, dy.ptr, n, d, None, None, _ffi.METRIC_DOT, do.ptr, None, ctypes.byref(form)) == 0
            eng.device_sync()
            out = do.numpy()
        finally:
            for a in (dx, dy, do):
                a.free()
        assert form.value == ref.form_of(n), (n, form.value)
        assert np.isnan(out[m]).all() and np.array_equal(_bits(out[:m]), _bits(want))
        seen.add(form.value)
    assert seen == {ref.FORM_128x64, ref.FORM_128x128}
    # the same element under both forms: columns 0 .. 2 of a 260-wide call (128 x 128) and the 3-wide call (128 x 64)
    x, y = ref.random_operands(200, 260, 160)
    assert np.array_equal(_bits(_run(eng, x, y[:3], _ffi.METRIC_DOT)), _bits(_run(eng, x, y, _ffi.METRIC_DOT))[:, :3])


def test_profiling_kind(eng):
    x, y = ref.random_operands(130, 70, 100)
    eng.profile(True)
    try:
        eng.profile_reset()
        eng.distmat(x, y, _ffi.METRIC_DOT, precision=X3)
        got = eng.profile_get(_ffi.K_DIST_GEMM)
    finally:
        eng.profile(False)
    assert got["launches"] == 1 and got["flops"] == 2.0 * 130 * 70 * 100


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
x = np.arange(12, dtype=np.float32).reshape(3, 4) / 7
before = eng.distmat(x, x, _ffi.METRIC_L2)
try:
    eng.distmat(x, x, _ffi.METRIC_L2, precision="f16x3")
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_distmat_x3.so" in str(e)
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.distmat(x, x, _ffi.METRIC_L2), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_distmat_x3.so, loaded through REID_HIP_LIB in a fresh child process: the fp32-class entry is
    REID_ERR_STATE naming the file before anything is launched, and the exact entry works before and after it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_distmat_x3.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED -3" in r.stdout and lib in r.stdout


# ---------------------------------------------------------------------------------------------- 8. rank sanity
@pytest.mark.parametrize("name", ("L2SQR", "COS"))
def test_argmin_agrees_where_float64_has_a_clear_winner(eng, name):
    """64 x 200 unit rows of width 512: on every row whose float64 top-2 gap exceeds the sum of both entries' bounds the arg-min of the new
    matrix is the exact entry's (and float64's); at most one row may be left out (the host test shows none is on this input).  A sanity
    check of the ranking, not a claim about bits."""
    metric = ref.METRICS[name]
    x, y = ref.rank_operands()
    best, clear = ref.rank_rows(x, y, metric)
    assert (~clear).sum() <= 1
    new = _run(eng, x, y, metric).argmin(1)
    exact = _run(eng, x, y, metric, precision=None).argmin(1)
    assert np.array_equal(new[clear], exact[clear]) and np.array_equal(new[clear], best[clear])
