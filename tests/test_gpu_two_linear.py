"""The fused pair of linears on the MI355X (pytest -m gpu tests/test_gpu_two_linear.py): two_linear_f16x3_kernel of csrc/two_linear_f16.hip
in its four builds (ACT, LN) against float64, through reid_debug_two_linear_form - launch_split_pack and launch_two_linear, the functions
the forward calls - with a guarded output and the context's fault status.  The oracle, the three views with their bounds, the exact
families and the case table are in tests/two_linear_ref.py; tests/test_two_linear_host.py holds them on the CPU and shows which
mutation of the arithmetic each view catches.
  1. every table row: status 0 and a clean fault word; view 1 (every hidden unit exposed through a 0/1 W2, one launch per C units) and
     view 3 (random W2: the composed sanity bound and the global figure of the old test) element by element; in the build without
     activation and LayerNorm the two exact families bit for bit; the 64 floats in front of the output and the 8 rows behind it untouched;
  2. the forward's aliasing (LN builds: x32 == res == out; packed builds: res == out) equals the separate-buffer launch bit for bit; the
     ragged in-place LN rows are run twice and agree - clamped lanes of a ragged block read row T - 1, which another wave may already be
     overwriting; their results are discarded but feed the range guards, and neither the output nor the fault word may depend on it;
  3. position invariance per build: copies of a row at another lane, wave, block, the first row of the ragged block and row T - 1;
  4. the two range guards (the hidden split's vmax, the normalised input's xmax) through the sticky software fault word;
  5. the launcher's refusals, with the output's fill pattern intact.

Each test prints its figures and the module ends with one "two_linear record" line per launch form; profiles/two_linear_gpu_tests.log is
that output of one run.

Recorded (one MI355X run; worst error / bound over the table's rows per launch form; a record, not the source of any constant):
  form                  view 1   view 3 (composed)   error over the well-conditioned rows / (1.5e-6 max |ref|)
  packed                0.020    0.0033              0.37
  packed-inplace        0.018    0.0024              0.41
  packed-gelu           0.021    0.0025              0.27
  packed-gelu-inplace   0.019    0.0022              0.33
  ln                    0.015    0.0043              0.41
  ln-inplace            0.082    0.0247              0.15
  ln-gelu               0.019    0.0043              0.33
  ln-gelu-inplace       0.080    0.0252              0.21
(the in-place LN forms sit higher because their residual is x itself: on the 300.0 spike of ln_rows' row 21 the sum's one rounding, half
an ulp of 300, is 0.08 of the SAFETY 4u |res| that dominates that element's bound; the emulation gives the same 0.082 there.)  The fp32 emulation of
tests/test_two_linear_host.py sits at 0.005 - 0.025 of view 1's bound and 0.0003 - 0.004 of view 3's.  The exact families were bit for
bit on every row without activation and LayerNorm; every in-place launch equalled its separate twin.  Nothing was found: the kernel and
the launcher are unchanged.
"""
import collections
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import two_linear_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu]
ERR_ARG, ERR_STATE = -1, -3
FILL = np.uint32(0xffffffff)
RECORD = collections.defaultdict(lambda: collections.defaultdict(float))     # launch form -> view -> worst error / bound


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    for form in sorted(RECORD):
        print("\ntwo_linear record %s: %s" % (form, ", ".join("%s %.4f" % kv for kv in sorted(RECORD[form].items()))))


@pytest.fixture(autouse=True)
def fp32_class(eng):
    """The kernel exists in precision 2 only; the context goes back to what it was."""
    before = eng.precision
    eng.set_precision(2)
    try:
        yield
    finally:
        eng.clear_fault()
        eng.set_precision(before)


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


def form_name(act, ln, alias):
    return "%s%s%s" % ("ln" if ln else "packed", "-gelu" if act else "", "-inplace" if alias else "")


def launch(eng, x, w1, b1, w2, b2, res, act=False, ln=None, alias=False, entered=True):
    """One harness call.  Checks the guard memory and returns (status, bits [m, c] uint32).  In the in-place LN form the residual is x.
    entered = False: a call the sticky fault word turns away on entry, which copies nothing back - the status alone."""
    m, c = x.shape
    if ln is not None and alias:
        assert res is x
        res = None
    st, raw, front = eng.debug_two_linear_form(x, w1, b1, w2, b2, res, act, ln, alias)
    if not entered:
        return st, None
    bits = raw.view(np.uint32)
    assert bits.size == front + (m + 8) * c
    assert (bits[:front] == FILL).all(), "memory in front of the output was written"
    body = bits[front:].reshape(m + 8, c)
    assert (body[m:] == FILL).all(), "rows >= m were written: %s" % np.unique(np.nonzero(body[m:] != FILL)[0])[:8]
    return st, np.ascontiguousarray(body[:m])


def values(bits):
    return bits.view(np.float32).astype(np.float64)


def row_operands(row):
    x, w1, b1, w2, b2, res, g, b = ref.operands(row.t, row.c, row.hid, row.ln)
    ln = (g, b) if row.ln else None
    return x, w1, b1, w2, b2, (x if row.ln and row.alias else res), ln


@functools.lru_cache(maxsize=4)
def row_hidden(row):
    x, w1, b1, _, _, _, ln = row_operands(row)
    return ref.hidden(x, w1, b1, row.act, ln)


def check_view3(bits, row, what):
    x, _, _, w2, b2, res, _ = row_operands(row)
    want, bd = ref.view3(row_hidden(row), w2, b2, res)
    got = values(bits)
    ratio = ref.check(got, want, bd, "two_linear v3 " + what)
    glob = float(np.abs(got - want)[ref.global_rows(x, row.ln)].max() / np.abs(want).max())
    print("two_linear v3 %s: max |err| over the well-conditioned rows %.3e of max |ref|" % (what, glob))
    assert glob <= ref.GLOBAL_TOL
    return ratio, glob / ref.GLOBAL_TOL


# ---------------------------------------------------------------------------------------------- 1. every table row against float64
@pytest.mark.parametrize("row", ref.TABLE, ids=ref.row_id)
def test_every_table_row(eng, row):
    what, form = ref.row_id(row), form_name(row.act, row.ln, row.alias)
    x, w1, b1, w2, b2, res, ln = row_operands(row)
    h = row_hidden(row)
    for off in ref.selection_offsets(row.c, row.hid):                                       # view 1: the hidden layer, C units per launch
        st, bits = launch(eng, x, w1, b1, ref.selection_w2(row.c, row.hid, off), b2, res, row.act, ln, row.alias)
        assert st == 0 and eng.fault_bits() == 0
        want, bd = ref.view1(h, row.c, off, b2, res)
        ratio = ref.check(values(bits), want, bd, "two_linear v1 %s off=%d" % (what, off))
        RECORD[form]["view1"] = max(RECORD[form]["view1"], ratio)
    st, bits = launch(eng, x, w1, b1, w2, b2, res, row.act, ln, row.alias)                  # view 3: both layers random
    assert st == 0 and eng.fault_bits() == 0
    ratio, glob = check_view3(bits, row, what)
    RECORD[form]["view3"] = max(RECORD[form]["view3"], ratio)
    RECORD[form]["global"] = max(RECORD[form]["global"], glob)
    if row.act or row.ln:
        return                                                                               # GELU and LayerNorm have no exact family
    ops = ref.exact_layer2(row.t, row.c, row.hid)                                            # view 2: layer 2 exact
    st, bits = launch(eng, *ops, alias=row.alias)
    want = ref.reference(*ops, False).astype(np.float32)
    bad = np.nonzero(bits.view(np.float32) != want)
    assert st == 0 and bad[0].size == 0, "exact layer 2: %d elements differ, first (%d, %d): %r against %r" % (
        bad[0].size, bad[0][0], bad[1][0], bits.view(np.float32)[bad][0], want[bad][0])
    for off in ref.selection_offsets(row.c, row.hid):                                        # ... and its mirror for layer 1
        ops = ref.exact_layer1(row.t, row.c, row.hid, off)
        st, bits = launch(eng, *ops, alias=row.alias)
        want = ref.reference(*ops, False).astype(np.float32)
        bad = np.nonzero(bits.view(np.float32) != want)
        assert st == 0 and bad[0].size == 0, "exact layer 1 off=%d: %d elements differ, first (%d, %d): %r against %r" % (
            off, bad[0].size, bad[0][0], bad[1][0], bits.view(np.float32)[bad][0], want[bad][0])
    assert eng.fault_bits() == 0
    print("two_linear exact %s: layer 2 and layer 1 families bit for bit" % what)


# ---------------------------------------------------------------------------------------------- 2. aliased and separate agree
@pytest.mark.parametrize("row", [r for r in ref.TABLE if r.alias], ids=ref.row_id)
def test_in_place_launch_equals_the_separate_one(eng, row):
    x, w1, b1, w2, b2, res, ln = row_operands(row)
    st, sep = launch(eng, x, w1, b1, w2, b2, res, row.act, ln, False)
    assert st == 0 and eng.fault_bits() == 0
    runs = 2 if row.ln and row.t in ref.RAGGED_IN_PLACE else 1
    for i in range(runs):
        st, inp = launch(eng, x, w1, b1, w2, b2, res, row.act, ln, True)
        assert st == 0 and eng.fault_bits() == 0, "in-place run %d: status %d, fault word %d" % (i, st, eng.fault_bits())
        assert np.array_equal(inp, sep), "in-place run %d differs from the separate launch in %d elements, rows %s" % (
            i, (inp != sep).sum(), np.unique(np.nonzero(inp != sep)[0])[:8])


# ---------------------------------------------------------------------------------------------- 3. position invariance
POS_T = 2 * ref.TOKENS_PER_BLOCK + 49                                                        # two full blocks and a ragged one
POS_SRC = 3
POS_DST = (9, 40, ref.TOKENS_PER_BLOCK + 67, 2 * ref.TOKENS_PER_BLOCK, POS_T - 1)            # lane, wave, block, first ragged row, row T - 1


@pytest.mark.parametrize("c", ref.CS)
@pytest.mark.parametrize("act,ln", ref.BUILDS, ids=lambda v: str(v))
def test_copies_of_a_row_give_equal_bits_wherever_they_sit(eng, act, ln, c):
    row = ref.Row(c, 4 * c if act else c, POS_T, act, ln, 0)
    x, w1, b1, w2, b2, res, lnp = row_operands(row)
    x, res = np.array(x), np.array(res)
    for dst in POS_DST:
        x[dst], res[dst] = x[POS_SRC], res[POS_SRC]
    for alias in ((0, 1) if ln else (0,)):                                                   # LN builds: the forward's in-place form too
        r = x if alias else res
        st, bits = launch(eng, x, w1, b1, w2, b2, r, act, lnp, alias)
        assert st == 0 and eng.fault_bits() == 0
        want, bd = ref.view3(ref.hidden(x, w1, b1, act, lnp), w2, b2, r)
        ref.check(values(bits), want, bd, "two_linear position %s c=%d" % (form_name(act, ln, alias), c))
        for dst in POS_DST:
            assert np.array_equal(bits[dst], bits[POS_SRC]), "row %d differs from its copy %d in %d elements" % (
                dst, POS_SRC, (bits[dst] != bits[POS_SRC]).sum())


# ---------------------------------------------------------------------------------------------- 4. range guards
def _raises(eng, call):
    st, _ = call(True)
    assert st == ERR_STATE and eng.fault_bits() == 1
    st, _ = call(False)                                                                      # the word stays set until cleared
    assert st == ERR_STATE
    eng.clear_fault()
    assert eng.fault_bits() == 0


GUARD_ROW = ref.Row(96, 96, 33, 0, 0, 0)


@pytest.mark.parametrize("act", (0, 1), ids=("plain", "gelu"))
def test_hidden_value_outside_f16_raises_the_fault_word(eng, act):
    """vmax: a hidden value of 7e4 (through b1) raises the sticky word with and without GELU (GELU(7e4) = 7e4); 6.5e4 does not, and the
    launch is still inside the composed bound."""
    x, w1, b1, w2, b2, res, _ = row_operands(GUARD_ROW)
    big = np.array(b1)
    big[40] = 7e4
    _raises(eng, lambda e: launch(eng, x, w1, big, w2, b2, res, act, entered=e))
    big[40] = 6.5e4
    assert np.abs(x.astype(np.float64) @ w1[40].astype(np.float64)).max() < 500
    st, bits = launch(eng, x, w1, big, w2, b2, res, act)
    assert st == 0 and eng.fault_bits() == 0
    want, bd = ref.view3(ref.hidden(x, w1, big, act), w2, b2, res)
    ref.check(values(bits), want, bd, "two_linear 6.5e4 hidden act=%d" % act)


@pytest.mark.parametrize("act", (0, 1), ids=("plain", "gelu"))
def test_normalised_input_outside_f16_raises_the_fault_word(eng, act):
    """xmax: a gamma of 1e6 drives |LN(x)| past 65504 on every row that is not constant."""
    row = GUARD_ROW._replace(ln=1, act=act)
    x, w1, b1, w2, b2, res, (g, b) = row_operands(row)
    big = np.array(g)
    big[5] = 1e6
    y = ref.ln_model(x, big, b, ref.LN_EPS, ref.ln_depth(row.c))[0]
    assert np.abs(y).max() >= 65504
    for alias in (0, 1):
        _raises(eng, lambda e: launch(eng, x, w1, b1, w2, b2, x if alias else res, act, (big, b), alias, entered=e))


@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("ln", (0, 1), ids=("packed", "ln"))
def test_non_finite_input_row_raises_the_fault_word_and_clean_rows_follow(eng, ln, bad):
    row = GUARD_ROW._replace(ln=ln, act=1)
    x, w1, b1, w2, b2, res, lnp = row_operands(row)
    x = np.array(x)
    x[17, 29] = bad
    _raises(eng, lambda e: launch(eng, x, w1, b1, w2, b2, res, 1, lnp, entered=e))
    row = next(r for r in ref.TABLE if r.ln == ln and r.t == 129)                            # after clear_fault a table row is correct and clean again
    x, w1, b1, w2, b2, res, lnp = row_operands(row)
    st, bits = launch(eng, x, w1, b1, w2, b2, res, row.act, lnp, row.alias)
    assert st == 0 and eng.fault_bits() == 0
    check_view3(bits, row, "after clear_fault " + ref.row_id(row))


# ---------------------------------------------------------------------------------------------- 5. refusals
def _refusal_operands(c, hid, t=33):
    rng = np.random.default_rng([c, hid])
    f = np.float32
    return [rng.normal(size=s).astype(f) for s in ((t, c), (hid, c), (hid,), (c, hid), (c,), (t, c))], (np.ones(c, f), np.zeros(c, f))


def _refused(eng, c, hid):
    ops, lnp = _refusal_operands(c, hid)
    for ln in (None, lnp):
        st, raw, _ = eng.debug_two_linear_form(*ops, act=True, ln=ln)
        assert st == ERR_ARG, "c=%d hid=%d ln=%d: status %d" % (c, hid, ln is not None, st)
        assert (raw.view(np.uint32) == FILL).all(), "a refused launch wrote its output"
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("c,hid", [(128, 128), (384, 384), (96, 48), (96, 4 * 96 + 32), (192, 4 * 192 + 32)], ids=str)
def test_refused_shapes(eng, c, hid):
    """launch_two_linear's ARG_CHECK on two_linear_supported: C other than 96 / 192, hid no multiple of 32, hid > 4 C"""
    _refused(eng, c, hid)


def test_refused_modes_and_the_context_still_works(eng):
    for precision in (0, 1):
        eng.set_precision(precision)
        try:
            _refused(eng, 96, 96)
        finally:
            eng.set_precision(2)
    with switches(eng, swin_two_linear=0):
        _refused(eng, 96, 384)
        _refused(eng, 192, 192)
    x, w1, b1, w2, b2, res, _ = row_operands(GUARD_ROW)
    st, bits = launch(eng, x, w1, b1, w2, b2, res)
    assert st == 0 and eng.fault_bits() == 0
    check_view3(bits, GUARD_ROW, "after the refusals")
