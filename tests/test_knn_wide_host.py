"""Host side of the large k-NN path's tests (no GPU): tests/knn_wide_ref.py held to itself, so that what tests/test_gpu_knn_wide.py asserts
on the device is not vacuous.
  1. the restatement returns the oracle's selection on every family, and three mutations are caught on an input built for each: a proof
     without its bound on the noisy-tie family, a selection that never looks at the last n % 4 columns, a bound without its absolute term
     on the outlier family (the premise, not the answer: N(0, 1) rows have gaps no error of that size closes);
  2. the conditions the GPU tests put on their inputs: the plain rows of the table are all clear at offsets 0 and 10, the copied-query rows
     of the near-tie families are not, the tie families' rows are tied from the k-th to the 32nd value;
  3. matching_ref.select_form agrees with the eligibility rule at its edges; the scales' restatement at an exact power of two;
  4. the harness is declared, bound and exported."""
import ctypes
import os
import sys

import numpy as np
import pytest

from reid_amd import _ffi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_wide_ref as ref  # noqa: E402
import matching_ref as mref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (9, 4097, 128)


def _wrong_rows(x, y, k, **kw):
    D, I, flagged, cand = ref.run(x, y, k, **kw)
    Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
    return (I != Iw).any(1) | (D != Dw).any(1), flagged


# ---------------------------------------------------------------------------------------------- 1. restatement and mutations
@pytest.mark.parametrize("family", ref.ROUNDED_FAMILIES)
def test_restated_path_selects_what_the_oracle_selects(family):
    x, y = ref.rounded_family(family, *SMALL)
    for k in (1, 5, 24):
        wrong, _ = _wrong_rows(x, y, k)
        assert not wrong.any(), (family, k, np.flatnonzero(wrong))


def test_proof_without_its_bound_returns_a_wrong_row_on_the_noisy_ties():
    """40 gallery rows within 2^-20 of each query: with err = 0 rows pass the proof and come back with neighbours the oracle does not list;
    with the stated bound every row is flagged and answered exactly."""
    x, y, slots = ref.noisy_tie_operands(*SMALL)
    for k in (5, 24):
        wrong0, flagged0 = _wrong_rows(x, y, k, err_on=False)
        assert wrong0.any() and (wrong0 & ~flagged0).any(), k
        wrong, flagged = _wrong_rows(x, y, k)
        assert not wrong.any() and flagged.all(), k
        Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)[1]
        assert all(set(Iw[i]) <= set(slots[i]) | {SMALL[1] - 1} for i in range(x.shape[0]))      # (the last column copies the last query)


@pytest.mark.parametrize("n", [nb for nb in ref.NBS if nb % 4])
def test_dropping_the_ragged_tail_changes_the_answer(n):
    """Every family puts a zero distance into the last column (x[m - 1] = y[n - 1]): a selection that stops at n & ~3 loses it."""
    for x, y in (mref.exact_operands(9, n, 128), ref.plain_operands(9, n, 128)):
        Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), 5)[1]
        assert Iw[-1, 0] == n - 1
        wrong, _ = _wrong_rows(x, y, 5, drop_tail=True)
        assert wrong.any()
        assert not _wrong_rows(x, y, 5)[0].any()


def test_the_relative_bound_alone_misses_the_outlier_rows():
    """One query 2^24 above the others sets sx: the others' scaled components lie near 2^-28, their high parts are zero and their low parts
    f16 subnormals of a few bits.  The restated matrix is then off by two orders of magnitude more than err_scale (|x|^2 + max |y|^2) sx sy;
    with err_abs = ld 2^-32 (derived in tests/knn_wide_ref.py) it is inside, as on every other family."""
    worst = {}
    for family in ref.ROUNDED_FAMILIES:
        x, y = ref.rounded_family(family, *SMALL)
        sx, sy, ss, my = ref.scales(x, y)
        diff = np.abs(ref.candidate_matrix(x, y).astype(np.float32).astype(np.float64) - ref.true_values(x, y, ss))
        rel = ref.row_err(ref.sqnorms(x), my, ss, 128, absolute=False)[:, None]
        full = ref.row_err(ref.sqnorms(x), my, ss, 128)[:, None]
        with np.errstate(all="ignore"):
            worst[family] = (float(np.nan_to_num(diff / rel).max()), float((diff / full).max()))
    print(" ".join("%s %.3g/%.3g" % ((f,) + v) for f, v in worst.items()))
    assert worst["outlier_q24"][0] > 10.0
    assert all(v[1] <= 1.0 for v in worst.values()), worst
    assert all(v[0] <= 1.0 for f, v in worst.items() if not f.startswith("outlier")), worst


@pytest.mark.parametrize("family", ("nan", "inf"))
def test_non_finite_norms_send_the_whole_call_through_the_rule(family):
    """(The overflow family's squares are finite in float64: there only the device's own matrix can be the reference.)"""
    x, y = ref.nonfinite_family(family)
    for k in (1, 5):
        D, I, flagged, _ = ref.run(x, y, k)
        Dw, Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)
        assert flagged.all() and np.array_equal(I, Iw) and np.array_equal(D, Dw)
        assert (I[1] == -1).all() and np.isposinf(D[1]).all() and (I != 2).all() and (family != "inf" or (I != 4).all())


# ---------------------------------------------------------------------------------------------- 2. conditions on the inputs
@pytest.mark.parametrize("row", ref.TABLE, ids=lambda r: "%dx%dx%d-k%d" % r[:4])
@pytest.mark.parametrize("offset", (0.0, 10.0))
def test_plain_rows_of_the_table_are_all_clear(row, offset):
    nq, nb, d, k, _ = row
    x, y = ref.plain_operands(nq, nb, d, offset)
    clear, gap, four = ref.clear_rows(x, y, k)
    print("%dx%dx%d k %d offset %g: smallest gap %.3g, largest 4 err %.3g" % (nq, nb, d, k, offset, gap.min(), four.max()))
    assert clear.all(), (gap.min(), four.max())


def test_near_tie_rows_are_not_clear_and_tie_families_are_tied():
    for k in (1, 5, 24):
        x, y = ref.rounded_family("near_tie", *SMALL)           # every query is copied some 65 times: d(k) = d(32) = 0
        assert not ref.clear_rows(x, y, k)[0].any() and ref.tied_rows(x, y, k).all()
        x, y, _ = ref.noisy_tie_operands(*SMALL)
        assert not ref.clear_rows(x, y, k)[0].any() and not ref.tied_rows(x, y, k).any()
        x, y = ref.identical_operands(*SMALL)
        assert ref.tied_rows(x, y, k).all()
        x, y, where = ref.copies_operands(*SMALL)
        assert ref.tied_rows(x, y, k).all() and len(where) > ref.CAP and where[-1] == SMALL[1] - 1
        Iw = ref.select(ref.oracle(x, y, ref.METRIC_L2SQR), k)[1]
        assert np.array_equal(Iw, np.tile(where[:k], (SMALL[0], 1)))
    for k in (5, 24):
        x, y = ref.straddle_operands(*SMALL, k)
        s = np.sort(ref.oracle(x, y, ref.METRIC_L2SQR), axis=1)
        assert (s[:, k - 2] == 0).all() and (s[:, k - 1:k + 39] == 1).all() and (s[:, k + 39] > 1).all()
        assert ref.tied_rows(x, y, k).all()
        assert not _wrong_rows(x, y, k)[0].any() and _wrong_rows(x, y, k)[1].all()


def test_survivor_counts_of_the_tie_families_cross_the_cap():
    """identical gallery and 1100 copies: more than CAP survivors in every row (the row is flagged by rowsel itself); 40 ties: fewer."""
    for (x, y), over in ((ref.identical_operands(*SMALL), True), (ref.copies_operands(*SMALL)[:2], True), (ref.straddle_operands(*SMALL, 5), False)):
        _, survivors, overflow = ref.rowsel(ref.candidate_matrix(x, y).astype(np.float32))
        assert overflow.all() if over else (not overflow.any() and (survivors >= ref.KK).all()), survivors


# ---------------------------------------------------------------------------------------------- 3. dispatch and scales
def test_select_form_agrees_with_the_eligibility_rule_at_its_edges():
    def eligible(nq, nb, d, k, wide_min):
        return 1 <= k <= ref.KMAX and nb >= ref.NB_MIN and d >= ref.D_MIN and nq * nb >= wide_min
    for inside, outside in ref.EDGES:
        wide_min = inside[0] * inside[1]
        for shape, want in ((inside, True), (outside, False)):
            assert eligible(*shape, wide_min) == want
            assert (mref.select_form(*shape, knn_wide_min=wide_min) == mref.WIDE) == want, shape
    nq, nb, d, k = 9, 4097, 128, 5
    assert mref.select_form(nq, nb, d, k, knn_wide_min=nq * nb) == mref.WIDE
    # nine queries are fewer than the fused search takes (m n >= 2^18): without the wide path they go through the matrix
    assert mref.select_form(nq, nb, d, k, knn_wide_min=nq * nb + 1) == mref.TWO_PASS_TOPK
    assert mref.select_form(nq, nb, d, k) == mref.TWO_PASS_TOPK and mref.select_form(8192, 4096, 128, k) == mref.WIDE
    assert mref.select_form(ref.FUSED_NQ, nb, d, k, knn_wide=0, knn_wide_min=1) == mref.FUSED_SELECT
    assert mref.select_form(ref.FUSED_NQ, nb, d, k, knn_wide_min=1) == mref.WIDE
    assert all(mref.select_form(r[0], r[1], r[2], r[3], knn_wide_min=1) == mref.WIDE for r in ref.TABLE)
    assert all(mref.select_form(r[0], r[1], r[2], r[3], knn_wide=0) == (mref.FUSED_SELECT if r[0] == 300 else mref.TWO_PASS_TOPK) for r in ref.TABLE)


def test_scales_are_powers_of_two_that_bring_every_component_into_the_unit_interval():
    assert [ref.pow2_inv(v) for v in (1.0, 4.0, 3.9, 0.25, 0.0, np.inf, np.nan, 1e-30)] == [0.5, 0.25, 0.5, 1.0, 1.0, 1.0, 1.0, 2.0 ** 49]
    assert ref.pow2_inv(2.0 ** 127) == 2.0 ** -64 and ref.pow2_inv(np.float32(1e-45)) == 2.0 ** 74
    for family in ref.ROUNDED_FAMILIES:
        x, y = ref.rounded_family(family, *SMALL)
        sx, sy, ss, my = ref.scales(x, y)
        assert np.abs(x).max() * sx <= 1.0 and np.abs(y).max() * sy <= 1.0
        assert family != "unit_max" or (sx, sy, my) == (0.5, 0.5, 1.0)
        assert family != "zero_queries" or sx == 1.0


# ---------------------------------------------------------------------------------------------- 4. the surface
def test_the_harness_is_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    dbg = ctypes.CDLL(_ffi.DEBUG_LIB_PATH)
    for sym in ("reid_debug_knn_wide_run", "reid_debug_knn_wide_eligible"):
        assert "int %s(" % sym in hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(dbg, sym), sym
    pub = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    comment = pub[:pub.index("int reid_knn(")].rsplit("/*", 1)[1]
    assert "expects finite operands" not in comment and "knn_wide.hip" in comment
