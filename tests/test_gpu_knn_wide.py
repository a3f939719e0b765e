"""The large k-NN path (csrc/knn_wide.hip) on the MI355X at the smallest shapes it accepts (pytest -m gpu tests/test_gpu_knn_wide.py), stage
by stage through reid_debug_knn_wide_run and as a whole through reid_knn*, against the float64 oracle and the restatement of
tests/knn_wide_ref.py (tests/test_knn_wide_host.py shows that those inputs can fail).  Every case lowers knn_wide_min to 1 through
Engine.debug_switch and restores it in a finally.
  a. exact family: D and I are the oracle's lexsort bit for bit at every n of the table, k = 1 / 5 / 24, nq = 1 / 9; all-equal gallery,
     1100 copies of the nearest row (both beyond CAP survivors: every row flagged), 40 columns tied across the 32nd candidate;
  b. rounded families: bit for bit the selection of the device's own distance matrix and the search without the wide path (two-pass at
     nine queries, the fused fp32 search at 72 and 300);
  c. the proof's premise: |matrix - sx sy (|y|^2 - 2 x.y)| <= err on every element, the true value in float64;
  d. the proof's verdicts: no clear row is flagged, every unflagged row's 32 keys hold the oracle's top k;
  e. rowsel_kernel: the returned keys are the 32 smallest of the returned matrix row by (key, column), at every n;
  f. query tiles: 300 rows in tiles of 256 equal the one-tile call, forced rows in the second tile included;
  g. dispatch at the edges of knn_wide_eligible, the product entry into guarded outputs;
  h. non-finite operands: the NaN rule of include/reid_hip.h, no fault bit, and the context goes on working.
Worst |matrix - true| / err as measured on the MI355X (profiles/knn_wide_gpu_tests.log), per family at (9, 4097, 128), with err_abs / against
the relative term alone:  n01 0.0311 / 0.0313, offset10 0.143 / 0.144, scale2m13 0.0311 / 0.0313, scale300 0.056 / 0.0565,
outlier_q14 0.00198 / 0.196, outlier_q24 0.00203 / 219, outlier_y14 0.0252 / 0.0252, zero_rows 0.0311 / 0.0313, zero_queries 0.0271 / 0.0271,
unit_max 0.0128 / 0.0132, near_tie 0.0878 / 0.0883, noisy_tie 0.133 / 0.134; the plain rows of the table 0.031 .. 0.091 at offset 0 and
0.10 .. 0.169 at offset 10 (the largest at 300 x 4351 x 128).  The 219 of outlier_q24 is the finding behind err_abs: the proof's bound was the
relative term alone, and the device then flagged one of that family's nine rows; with err_abs it flags all nine.  nflagged at k = 5: 9 of 9
on outlier_q24, outlier_y14, near_tie and noisy_tie, 0 on every other family and on every plain row of the table."""
import contextlib
import os
import sys

import numpy as np
import pytest

from reid_amd.parallel import DevArray

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_wide_ref as ref  # noqa: E402
import matching_ref as mref  # noqa: E402

pytestmark = [pytest.mark.gpu]
SMALL = (9, 4097, 128)
ALL_SET = np.uint32(0xffffffff)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


@contextlib.contextmanager
def wide(eng, wide_min=1, enable=1, force=0):
    """knn_wide_min lowered (and the test switches of reid_debug_knn_wide set) for the block, everything restored behind it."""
    before = eng.debug_switch("knn_wide_min")
    try:
        eng.debug_switch("knn_wide_min", wide_min)
        eng.debug_knn_wide(enable, force)
        yield
    finally:
        eng.debug_knn_wide(1, 0)
        eng.debug_switch("knn_wide_min", before)


def _run(eng, x, y, k, tile_rows=0, stages=True, force=0):
    with wide(eng, force=force):
        out = eng.debug_knn_wide_run(x, y, k, tile_rows, stages)
    assert (out["guard_D"] == ALL_SET).all() and (out["guard_I"] == -1).all(), "the guard row behind D / I was written"
    return out


def _assert_equal(out, Dw, Iw, what=""):
    D, I = (out["D"], out["I"]) if isinstance(out, dict) else out
    assert np.array_equal(I, Iw), "%s first difference at %s" % (what, np.argwhere(I != Iw)[:1].tolist())
    assert np.array_equal(_bits(D), _bits(Dw)), what


@pytest.fixture(scope="module")
def device_matrix(eng):
    """reid_distmat_dev's L2SQR matrix of a pair of operands, once per pair."""
    cache = {}

    def get(key, x, y):
        if key not in cache:
            cache[key] = eng.distmat(x, y, mref.METRIC_L2SQR)
        return cache[key]
    return get


# ---------------------------------------------------------------------------------------------- a. exact family
@pytest.mark.parametrize("row", ref.TABLE[:6], ids=lambda r: "%dx%dx%d-k%d" % r[:4])
def test_exact_family_equals_the_oracle_bit_for_bit(eng, row):
    nq, nb, d, k, _ = row
    x, y = mref.exact_operands(nq, nb, d)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    out = _run(eng, x, y, k)
    _assert_equal(out, Dw, Iw)
    assert Iw[nq - 1, 0] == nb - 1 and out["D"][nq - 1, 0] == 0.0            # the zero in the last row and column
    sx, sy, ss, my = ref.scales(x, y)                                          # integer norms are exact in fp32: the scales are decided
    assert np.array_equal(out["sc"], np.array([sx, sy, ss, my], np.float32))
    # integers times powers of two: the three-product arithmetic is exact, the candidate matrix IS the scaled true value
    assert np.array_equal(out["mat"][:, :nb].astype(np.float64), ref.true_values(x, y, ss))
    tied = ref.tied_rows(x, y, k)
    assert out["nflagged"] >= tied.sum() and out["flags"][tied].all() and out["nflagged"] == out["flags"].sum()
    with wide(eng):
        _assert_equal(eng.knn(x, y, k), Dw, Iw, "reid_knn")


@pytest.mark.parametrize("nb", ref.NBS)
@pytest.mark.parametrize("k", (1, 5, 24))
def test_exact_family_at_every_n_and_k(eng, nb, k):
    nq, d = (1, 128) if nb == 4098 else (9, 128)
    x, y = mref.exact_operands(nq, nb, d)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    out = _run(eng, x, y, k, stages=False)
    _assert_equal(out, Dw, Iw)
    assert out["nflagged"] >= ref.tied_rows(x, y, k).sum()


@pytest.mark.parametrize("case", ("identical", "copies1100", "straddle40"))
@pytest.mark.parametrize("k", (1, 5, 24))
def test_ties_beyond_the_candidates_take_the_exact_rows(eng, case, k):
    """identical: every gallery row the same vector - all nb columns survive the threshold (> CAP), the answer is columns 0 .. k - 1;
    copies1100: 1100 copies of every query's nearest row, the last column among them; straddle40: k - 1 exact copies of each query and 40
    distinct rows at distance 1 - the tie at the k-th value runs across the 32nd candidate (k = 1: 40 rows tied for the minimum).  A row
    whose k-th and 32nd oracle values are equal cannot be proven: each must be flagged and answered by the exact-row kernel."""
    nq, nb, d = SMALL
    if case == "identical":
        x, y = ref.identical_operands(nq, nb, d)
    elif case == "copies1100":
        x, y, where = ref.copies_operands(nq, nb, d)
    else:
        x, y = ref.straddle_operands(nq, nb, d, k)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    tied = ref.tied_rows(x, y, k)
    assert tied.all()
    out = _run(eng, x, y, k)
    _assert_equal(out, Dw, Iw)
    assert out["nflagged"] >= tied.sum() and out["flags"].all()
    over = ref.rowsel(out["mat"], nb)[2]
    if case == "identical":
        assert np.array_equal(out["I"], np.tile(np.arange(k, dtype=np.int32), (nq, 1))) and over.all()
    elif case == "copies1100":
        assert np.array_equal(out["I"], np.tile(where[:k].astype(np.int32), (nq, 1))) and over.all()
    else:
        assert not over.any()
    with wide(eng):
        _assert_equal(eng.knn(x, y, k), Dw, Iw, "reid_knn")


# ---------------------------------------------------------------------------------------------- b - e. rounded families
@pytest.fixture(scope="module")
def family_runs(eng, device_matrix):
    """One stage run per (family, k) at (9, 4097, 128), shared by b - e."""
    cache = {}

    def get(family, k=5):
        if (family, k) not in cache:
            x, y = ref.rounded_family(family, *SMALL)
            cache[family, k] = (x, y, _run(eng, x, y, k), device_matrix(family, x, y))
        return cache[family, k]
    return get


@pytest.mark.parametrize("family", ref.ROUNDED_FAMILIES)
def test_rounded_families_equal_the_device_matrix_selection_and_the_other_paths(eng, family, family_runs):
    """(9, 4097, 128): the wide path, stage run and reid_knn, against `select` of reid_distmat_dev's matrix and against reid_knn with the wide
    path off - at nine queries the two-pass search; the same queries repeated to 72 rows reach the fused fp32 search (72 x 4097 >= 2^18)."""
    for k in (1, 5, 24):
        x, y, out, dev = family_runs(family, k)
        Dw, Iw = ref.select(dev, k)
        _assert_equal(out, Dw, Iw, "stage run k %d" % k)
        with wide(eng):
            _assert_equal(eng.knn(x, y, k), Dw, Iw, "reid_knn k %d" % k)
        with wide(eng, enable=0):
            _assert_equal(eng.knn(x, y, k), Dw, Iw, "two-pass k %d" % k)
    x, y, out, dev = family_runs(family, 5)
    reps = ref.FUSED_NQ // SMALL[0]
    x72 = np.ascontiguousarray(np.tile(x, (reps, 1)))
    Dw, Iw = (np.tile(a, (reps, 1)) for a in ref.select(dev, 5))
    assert mref.select_form(ref.FUSED_NQ, SMALL[1], SMALL[2], 5, knn_wide=0) == mref.FUSED_SELECT
    with wide(eng, enable=0):
        _assert_equal(eng.knn(x72, y, 5), Dw, Iw, "fused")
    with wide(eng):
        _assert_equal(eng.knn(x72, y, 5), Dw, Iw, "wide, 72 rows")
    if family in ("near_tie", "noisy_tie"):
        assert out["nflagged"] > 0
    print("%s: nflagged %d of %d (k = 5)" % (family, out["nflagged"], SMALL[0]))


@pytest.mark.parametrize("row", ref.TABLE, ids=lambda r: "%dx%dx%d-k%d" % r[:4])
@pytest.mark.parametrize("offset", (0.0, 10.0))
def test_plain_rows_of_the_table_are_proven_and_equal_the_fused_search(eng, row, offset):
    """The plain N(0, 1) rows (+ offset) at every shape of the table: all rows are clear (tests/test_knn_wide_host.py), so none may be flagged;
    D and I equal `select` of the device's matrix and the search without the wide path (fused at 300 queries); the premise holds."""
    nq, nb, d, k, _ = row
    x, y = ref.plain_operands(nq, nb, d, offset)
    out = _run(eng, x, y, k)
    Dw, Iw = ref.select(eng.distmat(x, y, mref.METRIC_L2SQR), k)
    _assert_equal(out, Dw, Iw)
    with wide(eng, enable=0):
        _assert_equal(eng.knn(x, y, k), Dw, Iw, mref.select_form(nq, nb, d, k, knn_wide=0))
    worst = _premise(out, x, y)
    print("plain %dx%dx%d k %d offset %g: nflagged %d, worst |mat - true| / err %.3g" % (nq, nb, d, k, offset, out["nflagged"], worst[0]))
    assert worst[0] <= 1.0
    _verdicts(out, x, y, k, nb)
    assert out["nflagged"] == 0 and not out["flags"].any()
    _rowsel_equals(out, nb)


def _premise(out, x, y):
    """(worst |mat - true| / err with err_abs, worst against the relative term alone), columns below nb, the device's own scales."""
    sx, sy, ss, my = (float(v) for v in out["sc"])
    nb, ld = y.shape[0], ref.ld_of(x.shape[1])
    assert np.frexp(sx)[0] == 0.5 and np.frexp(sy)[0] == 0.5 and np.abs(x).max() * sx <= 1.0 and np.abs(y).max() * sy <= 1.0 and ss == sx * sy
    r2 = ref.sqnorms(x)
    diff = np.abs(out["mat"][:, :nb].astype(np.float64) - ref.true_values(x, y, ss))
    full = ref.row_err(r2, my, ss, ld)[:, None]
    rel = ref.row_err(r2, my, ss, ld, absolute=False)[:, None]
    with np.errstate(all="ignore"):
        return float((diff / full).max()), float(np.nan_to_num(diff / rel, nan=0.0).max())


@pytest.mark.parametrize("family", ref.ROUNDED_FAMILIES)
def test_every_matrix_entry_is_within_the_proofs_bound(family, family_runs):
    """c.  The proof is sound only if every entry of the candidate matrix is within err of sx sy (|y|^2 - 2 x.y); the true value in float64,
    err = err_scale (|x|^2 + max |y|^2) sx sy + err_abs as tests/knn_wide_ref.py restates and derives it.  A ratio above 1 is a finding
    about the bound."""
    x, y, out, _ = family_runs(family)
    sx, sy, ss, my = ref.scales(x, y)
    assert float(out["sc"][0]) in (sx, sx / 2, sx * 2) and float(out["sc"][1]) in (sy, sy / 2, sy * 2)
    if family in ("unit_max", "zero_queries"):       # maxima that fp32 sums exactly in any order: the scales are decided
        assert np.array_equal(out["sc"], np.array([sx, sy, ss, my], np.float32))
    full, rel = _premise(out, x, y)
    print("%s: worst |mat - true| / err %.3g (relative term alone %.3g)" % (family, full, rel))
    assert full <= 1.0


def _verdicts(out, x, y, k, nb):
    sx, sy, ss, my = (float(v) for v in out["sc"])
    s = np.sort(ref.oracle(x, y, ref.METRIC_L2SQR), axis=1)
    four = 4.0 * ref.row_err(ref.sqnorms(x), my, ss, ref.ld_of(x.shape[1])) / ss
    clear = s[:, ref.KK - 1] - s[:, k - 1] > four
    flags = out["flags"] != 0
    assert not (clear & flags).any(), "clear rows %s were flagged" % np.flatnonzero(clear & flags)[:8]
    Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)[1]
    cand = ref.key_columns(out["keys"])
    for i in np.flatnonzero(~flags):
        assert set(Iw[i].tolist()) <= set(cand[i].tolist()), "row %d passed the proof without the oracle's top %d among its candidates" % (i, k)
    return clear, flags


@pytest.mark.parametrize("family", ref.ROUNDED_FAMILIES)
def test_the_proofs_verdicts(family, family_runs):
    """d.  No clear row is flagged; every row the proof passed has the oracle's top k among its 32 candidates.  The near-tie families' rows
    are not clear (host test) and have more near neighbours than candidates: they must be flagged."""
    for k in (1, 5, 24):
        x, y, out, _ = family_runs(family, k)
        clear, flags = _verdicts(out, x, y, k, SMALL[1])
        assert out["nflagged"] == flags.sum()
        if family in ("n01", "offset10", "scale2m13", "scale300", "zero_rows", "zero_queries", "unit_max"):
            assert clear.all() and not flags.any(), (family, k)
        if family in ("near_tie", "noisy_tie"):
            assert flags.all(), (family, k)
        print("%s k %d: clear %d, flagged %d of %d" % (family, k, clear.sum(), flags.sum(), len(flags)))


def _rowsel_equals(out, nb):
    keys, survivors, over = ref.rowsel(out["mat"], nb)
    ok = ~over
    assert np.array_equal(out["keys"][ok], keys[ok]), "rows %s" % np.flatnonzero((out["keys"] != keys).any(1) & ok)[:8]
    assert (out["flags"][over] != 0).all()
    return ok.sum()


@pytest.mark.parametrize("nb", ref.NBS)
def test_rowsel_returns_the_32_smallest_of_the_matrix_row(eng, nb):
    """e.  On the bits of the returned matrix: the returned keys are its 32 smallest per row by (key, column) - the last n % 4 columns, which
    rowsel_kernel reads apart from its 16-byte sweep, hold each row's smallest or near-smallest values in these families."""
    for name, (x, y) in (("plain", ref.plain_operands(9, nb, 128)), ("near_tie", ref.rounded_family("near_tie", 9, nb, 128)),
                         ("exact", mref.exact_operands(9, nb, 128))):
        out = _run(eng, x, y, 5)
        assert _rowsel_equals(out, nb) == 9, name
        assert name == "near_tie" or ref.key_columns(out["keys"])[8, 0] == nb - 1, "%s: the last column is not the last row's first candidate" % name
    x, y = (a.copy() for a in ref.plain_operands(9, nb, 128))
    for t in range(nb % 4):                          # every tail column a copy of a query: all of them must be candidates
        y[nb - 1 - t] = x[t]
    out = _run(eng, x, y, 5)
    assert _rowsel_equals(out, nb) == 9
    for t in range(nb % 4):
        assert out["I"][t, 0] == nb - 1 - t and nb - 1 - t in ref.key_columns(out["keys"])[t]


# ---------------------------------------------------------------------------------------------- f. query tiles
@pytest.mark.parametrize("force", (0, 7))
def test_two_query_tiles_equal_one(eng, force):
    """300 queries in tiles of 256 and 44 rows (flags, norms and outputs offset by the tile's first row) against the one-tile call and the
    selection of the device's matrix, and on the exact family against the oracle; force = 7: every seventh row takes the exact-row kernel, rows 259 .. 294 of them in the second tile."""
    nq, nb, d, k = 300, 4099, 136, 24
    x, y = ref.plain_operands(nq, nb, d)
    Dw, Iw = ref.select(eng.distmat(x, y, mref.METRIC_L2SQR), k)
    one = _run(eng, x, y, k, 0, True, force)
    two = _run(eng, x, y, k, 256, False, force)
    _assert_equal(one, Dw, Iw, "one tile")
    _assert_equal(two, Dw, Iw, "two tiles")
    want = len(range(0, nq, force)) if force else 0
    assert one["nflagged"] == two["nflagged"] == want
    x, y = mref.exact_operands(nq, nb, d)
    De, Ie = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    _assert_equal(_run(eng, x, y, k, 256, False, force), De, Ie, "exact family, two tiles")


# ---------------------------------------------------------------------------------------------- g. dispatch
def test_eligibility_and_answers_on_both_sides_of_every_edge(eng):
    for inside, outside in ref.EDGES:
        for shape in (inside, outside):
            nq, nb, d, k = shape
            with wide(eng):
                assert eng.debug_knn_wide_eligible(*shape) == (mref.select_form(*shape, knn_wide_min=1) == mref.WIDE) == (shape == inside)
                x, y = mref.exact_operands(nq, nb, d)
                _assert_equal(eng.knn(x, y, k), *ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k), what=str(shape))
    nq, nb, d, k = 9, 4097, 128, 5
    x, y = mref.exact_operands(nq, nb, d)
    want = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    for wide_min, is_wide in ((nq * nb, True), (nq * nb + 1, False)):
        with wide(eng, wide_min):
            assert eng.debug_knn_wide_eligible(nq, nb, d, k) == is_wide == (mref.select_form(nq, nb, d, k, knn_wide_min=wide_min) == mref.WIDE)
            _assert_equal(eng.knn(x, y, k), *want, what="knn_wide_min %d" % wide_min)
    assert eng.debug_switch("knn_wide_min") == ref.WIDE_MIN and not eng.debug_knn_wide_eligible(nq, nb, d, k)
    assert eng.debug_knn_wide_eligible(8192, 4096, 128, 24) and not eng.debug_knn_wide_eligible(8191, 4096, 128, 24)
    with wide(eng, enable=0):
        assert not eng.debug_knn_wide_eligible(nq, nb, d, k)


def test_product_entry_into_guarded_outputs(eng):
    """reid_knn_dev at (9, 4097, 128, 5) through the wide path into outputs with eight marked elements on either side."""
    nq, nb, d, k, g = 9, 4097, 128, 5, 8
    x, y = mref.exact_operands(nq, nb, d)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    mark = np.uint32(0x7fc0dead)
    dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
    d_D = DevArray.from_numpy(eng, np.full(nq * k + 2 * g, mark, np.uint32).view(np.float32))
    d_I = DevArray.from_numpy(eng, np.full(nq * k + 2 * g, -7, np.int32))
    try:
        with wide(eng):
            assert eng.debug_knn_wide_eligible(nq, nb, d, k)
            eng.knn_dev(dx.ptr, nq, dy.ptr, nb, d, k, d_D.ptr + 4 * g, d_I.ptr + 4 * g)
            eng.sync()
        D, I = d_D.numpy().view(np.uint32), d_I.numpy()
    finally:
        for a in (dx, dy, d_D, d_I):
            a.free()
    for a, m in ((D, mark), (I, -7)):
        assert (a[:g] == m).all() and (a[-g:] == m).all(), "an element beside the output was written"
    assert np.array_equal(I[g:-g].reshape(nq, k), Iw) and np.array_equal(D[g:-g].reshape(nq, k), _bits(Dw))


# ---------------------------------------------------------------------------------------------- h. non-finite operands
@pytest.mark.parametrize("family", ref.NONFINITE_FAMILIES)
def test_nan_rule_holds_on_the_wide_path(eng, family):
    """A NaN (sign clear) in query 1, a NaN (sign set) in gallery row 2, zero rows; `inf`: a +inf component in gallery row 4; `overflow`: a
    query whose squared norm is +inf in fp32.  reid_knn through the wide path answers what `select` makes of the device's own matrix - a NaN
    distance no candidate, the all-NaN row (+inf, -1) - with the bits of the search without the wide path (two-pass at 9, fused at 72
    queries), raises no fault bit (reid_knn is an exact-fp32 entry), and a finite search behind it returns what it returned before."""
    x, y = ref.nonfinite_family(family)
    nq, nb, d = x.shape[0], y.shape[0], x.shape[1]
    xf, yf = ref.plain_operands(nq, nb, d)
    reps = ref.FUSED_NQ // nq
    x72 = np.ascontiguousarray(np.tile(x, (reps, 1)))
    try:
        with wide(eng):
            before = eng.knn(xf, yf, 5)
        dev = eng.distmat(x, y, mref.METRIC_L2SQR)
        assert np.isnan(dev[1]).all() and np.isnan(dev[:, 2]).all()
        for k in (1, 5, 24):
            Dw, Iw = ref.select(dev, k)
            assert (Iw[1] == -1).all() and (Iw != 2).all()
            with wide(eng):
                assert eng.debug_knn_wide_eligible(nq, nb, d, k)
                got = eng.knn(x, y, k)
                bits = eng.fault_bits()
            _assert_equal(got, Dw, Iw, "wide k %d" % k)
            assert bits == 0, "fault bits %d" % bits
            with wide(eng, enable=0):
                _assert_equal(eng.knn(x, y, k), Dw, Iw, "two-pass k %d" % k)
        Dw, Iw = (np.tile(a, (reps, 1)) for a in ref.select(dev, 5))
        with wide(eng, enable=0):
            _assert_equal(eng.knn(x72, y, 5), Dw, Iw, "fused")
        with wide(eng):
            _assert_equal(eng.knn(x72, y, 5), Dw, Iw, "wide, 72 rows")
            out = eng.debug_knn_wide_run(x, y, 5, 0, False)
            _assert_equal(out, *ref.select(dev, 5), what="stage run")
            assert (out["guard_D"] == ALL_SET).all() and (out["guard_I"] == -1).all()
            assert out["nflagged"] == nq                 # a non-finite norm: every row of the call is answered by the exact-row kernel
            assert eng.fault_bits() == 0
            after = eng.knn(xf, yf, 5)
        assert np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[0]), _bits(before[0]))
        if family == "overflow":
            assert np.isposinf(dev[3, [0, 1, 3]]).all() and Iw[3].tolist() == [0, 1, 3, 4, 5]
        if family == "inf":
            assert np.isposinf(dev[0, 4]) or np.isnan(dev[0, 4])
    finally:
        if eng.fault_bits():
            eng.clear_fault()
