"""Host-side checks of tests/matching_ref.py (no GPU): the exact family is exact, the fp32 restatements of oracle/matching.py agree with the
float64 oracle the GPU tests use, the rounded family's bound holds for the reference before it is asked of a kernel, the dispatch
predicates reach every launch form, and the selection oracle is the rule it claims to be."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_ref as ref  # noqa: E402
from oracle import matching  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _exact_inputs():
    seen = set()
    for m, n, d in [r[:3] for r in ref.DIST_TABLE] + [r[:3] for r in ref.SELECT_TABLE]:
        if (m, n, d) not in seen:
            seen.add((m, n, d))
            yield ref.exact_operands(m, n, d)
    for m, n, d, k, identical, _ in ref.SELECT_TABLE:
        if identical and (m, n, d, 1) not in seen:
            seen.add((m, n, d, 1))
            yield ref.exact_operands(m, n, d, True)
    xq, xb, _ = ref.one_thread_operands()
    yield xq, xb


def test_exact_family_stays_below_2_to_24():
    """Integers of magnitude <= 4: the sums of magnitudes of a dot product, of a squared norm and of |x|^2 + |y|^2 + 2 |x.y| bound every
    partial sum in any order; all stay below 2^24, so fp32 holds each intermediate exactly."""
    for x, y in _exact_inputs():
        assert x.shape[1] <= 2048 and np.abs(x).max() <= 4 and np.abs(y).max() <= 4
        assert np.array_equal(x, np.rint(x)) and np.array_equal(y, np.rint(y))
        ax, ay = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
        s = (ax * ax).sum(1)[:, None] + (ay * ay).sum(1)[None, :] + 2.0 * (ax @ ay.T)
        assert s.max() < 2.0 ** 24
        for metric in (ref.METRIC_DOT, ref.METRIC_L2SQR):
            v = ref.oracle(x, y, metric)
            assert np.array_equal(v, np.rint(v)) and np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_fp32_restatements_reproduce_the_float64_oracle_on_the_exact_family():
    """oracle/matching.py in float32 (numpy's summation order) gives the float64 oracle's values bit for bit - exact in one fp32 order,
    and by the magnitude argument in any: x @ y.T for DOT, euclidean_dist for L2 (sqrt is correctly rounded in both widths, and rounding
    float64's root to float32 is innocuous: 53 >= 2 * 24 + 2), knn_l2sqr for L2SQR and for the selection oracle's order."""
    for x, y in _exact_inputs():
        if x.shape[0] * y.shape[0] > 1 << 18:            # the restatements are quadratic in memory and the argument does not depend on size
            x, y = x[:40], y[:600]
        assert np.array_equal(_bits(x @ y.T), _bits(ref.oracle(x, y, ref.METRIC_DOT)))
        assert np.array_equal(_bits(matching.euclidean_dist(x, y)), _bits(ref.oracle(x, y, ref.METRIC_L2)))
        n = y.shape[0]
        D, I = matching.knn_l2sqr(x, y, n)
        Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), n)
        assert np.array_equal(I, Iw) and np.array_equal(_bits(D), _bits(Dw))
        if x.shape[1] > 1:                               # d = 1 holds zeros: 0 / 0
            assert ref.exact_mismatch(matching.cosine_dist(x, y), x, y, ref.METRIC_COS_HALF) == 0


def test_exact_family_has_real_ties():
    x, y = ref.exact_operands(128, 2049, 64)
    v = ref.oracle(x, y, ref.METRIC_L2SQR)
    assert v[0, 3] == 0 and v[0, 2049 // 2] == 0 and v[127, 2048] == 0
    distinct_rows_tied = sum(len(np.unique(row)) < len(row) - 1 for row in v)
    assert distinct_rows_tied == 128                     # every row has distinct gallery rows at equal distance
    D, I = ref.select(v, 7)
    assert I[0, 0] == 3 and I[0, 1] == 2049 // 2 and (np.diff(D, axis=1) == 0).any()
    xi, yi = ref.exact_operands(128, 2049, 64, True)
    assert (yi == yi[0]).all() and np.array_equal(ref.select(ref.oracle(xi, yi, ref.METRIC_L2SQR), 20)[1], np.tile(np.arange(20, dtype=np.int32), (128, 1)))


@pytest.mark.parametrize("name", sorted(ref.METRICS))
def test_cosine_winners_are_decided_on_at_least_nine_rows_in_ten(name):
    """The arg-min of the exact family is asserted on the index for every metric; under the cosine forms only where float64's winner leads
    by more than twice the allowance.  The seed of exact_operands was chosen so that the oracle alone decides >= 90 % of the rows."""
    for m, n, d, k, identical, _ in ref.SELECT_TABLE:
        if identical or n < 2:
            continue
        x, y = ref.exact_operands(m, n, d)
        assert ref.enough_decided(ref.decided_rows(x, y, ref.METRICS[name])), (m, n, d)


def test_rounded_family_restatement_stays_inside_the_bound():
    """The bound of the module docstring holds for numpy's float32 arithmetic (another summation order than the kernels') on every shape
    and offset the GPU test uses; the largest share is printed."""
    worst = {}
    for m, n, d, *_ in ref.ROUNDED_TABLE:
        for offset in (0.0, 10.0):
            x, y = ref.rounded_operands(m, n, d, offset)
            xx = (x * x).sum(1, dtype=np.float32)[:, None]
            yy = (y * y).sum(1, dtype=np.float32)[None, :]
            dot = x @ y.T
            l2sqr = (xx + yy) + np.float32(-2.0) * dot
            got = {"DOT": dot, "L2SQR": l2sqr, "L2": matching.euclidean_dist(x, y), "COS_HALF": matching.cosine_dist(x, y),
                   "COS": np.float32(2.0) * matching.cosine_dist(x, y)}
            for name, g in got.items():
                share = ref.rounded_share(g, x, y, ref.METRICS[name])
                worst[name] = max(worst.get(name, 0.0), share)
                assert share <= 1.0, (name, m, n, d, offset, share)
    print("float32 restatement, largest err / bound:", {k: "%.3g" % v for k, v in sorted(worst.items())})
    assert min(worst.values()) > 1e-3                    # the bound is not vacuous: numpy's own rounding uses a visible part of it


def test_bound_notices_an_operand_rounded_to_f16():
    x, y = ref.rounded_operands(129, 65, 96, 10.0)
    xh, yh = x.astype(np.float16).astype(np.float32), y.astype(np.float16).astype(np.float32)
    for name in ("DOT", "L2SQR", "L2"):
        got = ref.oracle(xh, yh, ref.METRICS[name])
        assert ref.rounded_share(got, x, y, ref.METRICS[name]) > 1.0, name


def test_dispatch_predicates_reach_every_form():
    reached = set()
    for m, n, d, x_off, out_off, f32_conv, bk16, form in ref.DIST_TABLE:
        assert ref.dist_form(m, n, d, x_off, f32_conv, bk16) == form, (m, n, d, x_off, f32_conv, bk16)
        full, ragged, ntiles, last = ref.dist_tiles(m, n, form)
        reached.add((form, "full" if full else "", "ragged" if ragged else "", "edge" if last not in (64, 128) else ""))
    for form in ref.DIST_FORMS:
        # a full 128-row tile (the buffer-store branch) beside a ragged one with a column edge, and a ragged-only tile
        assert (form, "full", "ragged", "edge") in reached, form
        assert any(r[0] == form and not r[1] for r in reached), form
    assert (ref.DMA64, "full", "", "") in reached and (ref.DMA64, "full", "", "edge") in reached
    # what the column rule does at the table's widths
    assert [ref.dist_form(129, n, 32) for n in (1, 64, 65, 129, 193)] == [ref.DMA64, ref.DMA64, ref.DMA128_K16, ref.DMA64, ref.DMA128_K16]
    assert ref.dist_tiles(129, 129, ref.DMA64) == (1, 1, 3, 1) and ref.dist_tiles(129, 193, ref.DMA128_K16) == (1, 1, 2, 65)
    # the copy of pad_rows: d % 4 != 0, or a pointer off 16 bytes
    assert ref.padded_k(1) == (4, True) and ref.padded_k(33) == (36, True) and ref.padded_k(32, 1) == (32, True) and ref.padded_k(32) == (32, False)
    assert any(ref.padded_k(d, xo)[1] and form.startswith("dma") for _, _, d, xo, _, _, _, form in ref.DIST_TABLE)
    # the shape of the older k16 / k32 case, n = 257, takes the 64-wide tile under both switches: it compared a kernel with itself
    assert ref.dist_form(300, 257, 512, bk16=0) == ref.dist_form(300, 257, 512, bk16=1) == ref.DMA64

    seen = set()
    for m, n, d, k, identical, form in ref.SELECT_TABLE:
        assert ref.select_form(m, n, d, k) == form, (m, n, d, k)
        assert ref.select_form(m, n, d, k, two_pass=1) == ref.TWO_PASS_TOPK
        seen.add(form)
        seen.add(ref.select_form(m, n, d, 1, entry="argmin"))
        if form in (ref.FUSED_ARGMIN, ref.FUSED_SELECT):
            nnt, S = (n + 127) // 128, ref.select_segments(m, n)
            seen.add((form, "tiles per segment", (nnt + S - 1) // S, "row tiles", (m + 127) // 128))
    assert set(ref.SELECT_FORMS) <= seen and ref.WIDE not in seen
    assert ref.select_segments(128, 2049) == 17 and ref.select_segments(70, 4200) == 17 and ref.select_segments(129, 2049) == 17
    for form in (ref.FUSED_ARGMIN, ref.FUSED_SELECT):
        assert (form, "tiles per segment", 1, "row tiles", 1) in seen and (form, "tiles per segment", 2, "row tiles", 1) in seen
    assert (ref.FUSED_SELECT, "tiles per segment", 1, "row tiles", 2) in seen
    for m, n, d in ref.NONFINITE_SHAPES:
        assert ref.select_form(m, n, d, 5) == (ref.TWO_PASS_TOPK if n < 2048 else ref.FUSED_SELECT)
    xq, xb, _ = ref.one_thread_operands()
    assert ref.select_form(xq.shape[0], xb.shape[0], 32, 10) == ref.TWO_PASS_TOPK
    # the wide path stays out of every row (d = 64 < 128); it would take a Market-size search
    assert ref.select_form(3368, 15913, 512, 20) == ref.WIDE and ref.select_form(3368, 15913, 64, 20) == ref.FUSED_SELECT


def test_selection_oracle_is_a_plain_sort_with_the_nan_rule():
    nan_neg, nan_pos = ref.NAN_NEG, ref.NAN_POS
    assert np.signbit(nan_neg) and not np.signbit(nan_pos) and np.isnan(nan_neg) and np.isnan(nan_pos)
    mat = np.array([[3.0, 1.0, nan_neg, 1.0, -np.inf, np.inf, nan_pos, 1.0],
                    [nan_neg, nan_pos, nan_neg, nan_pos, nan_neg, nan_pos, nan_neg, nan_pos],
                    [2.0, nan_pos, 2.0, 2.0, nan_neg, -0.0, 0.0, np.inf]], np.float32)
    for k in (1, 3, 8, 10):
        D, I = ref.select(mat, k)
        for i, row in enumerate(mat.tolist()):
            cand = sorted((v, j) for j, v in enumerate(row) if v == v)[:k]          # Python's tuple order: value, then column
            assert I[i].tolist() == [j for _, j in cand] + [-1] * (k - len(cand))
            assert D[i, :len(cand)].tolist() == [v for v, _ in cand] and np.isposinf(D[i, len(cand):]).all()
    idx, val = ref.argmin_rule(mat)
    assert idx.tolist() == [4, -1, 5] and val[0] == -np.inf and np.isnan(val[1]) and val[2] == 0.0
    x, y = ref.nan_gallery_operands()
    D, I = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), 4)
    assert sorted(I[0].tolist()) == [-1, -1, 1, 4] and (I[1] == -1).all() and np.isposinf(D[1]).all()


def test_nonfinite_family_is_what_it_says():
    for m, n, d in ref.NONFINITE_SHAPES:
        x, y = ref.nonfinite_operands(m, n, d, True)
        assert np.isnan(x[1]).sum() == 1 and not np.signbit(x[1][np.isnan(x[1])][0])
        assert np.isnan(y[2]).sum() == 1 and np.signbit(y[2][np.isnan(y[2])][0])
        assert not x[m - 1].any() and not y[n - 1].any() and np.isposinf(y[4]).sum() == 1 and np.isneginf(y[n - 2]).sum() == 1
        v = ref.oracle(x, y, ref.METRIC_DOT)
        assert np.isnan(v[1]).all() and np.isnan(v[:, 2]).all() and np.isnan(v[m - 1, 4]) and np.isinf(v[0, 4]) and np.isinf(v[0, n - 2])
        x, y = ref.nonfinite_operands(m, n, d)
        c = ref.oracle(x, y, ref.METRIC_COS)
        assert np.isnan(c[m - 1]).all() and np.isnan(c[:, n - 1]).all() and np.isfinite(c[0, 0])
        l2 = ref.oracle(x, y, ref.METRIC_L2)
        assert np.isnan(l2[1]).all() and np.isnan(l2[:, 2]).all() and np.isfinite(l2[m - 1, n - 1])
        assert np.isnan(ref.argmin_rule(l2)[1][1]) and ref.argmin_rule(l2)[0][1] == -1


def test_diou_cases_cover_the_edges():
    cases = ref.diou_cases()
    assert sorted(t.shape[0] * d.shape[0] for t, d in cases.values())[-3:] == [255, 256, 257]
    with np.errstate(all="ignore"):
        c = matching.diou_cost(*cases["touching_nested_zero"])
    assert np.isnan(c[5, 6]) and np.isnan(c[5, 5]) and np.isfinite(c[0, 1]) and np.isfinite(c[4, 0])
    assert (cases["negative"][0][:, :2] < 0).all() and cases["near_1e8"][0][:, :2].min() >= 1e8
