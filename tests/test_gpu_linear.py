"""The Linear layers on the MI355X (pytest -m gpu tests/test_gpu_linear.py): every launch form of linear() / linear16() (csrc/swin.hip) in
every precision against the float64 oracle of tests/linear_ref.py, through reid_debug_swin_linear - the forward's own functions, so each
case sees the forward's dispatch, operand preparation, padding and epilogue.  The error model, the dispatch predicates and the case table
(which row reaches which kernel and why) are in tests/linear_ref.py; tests/test_linear_host.py holds them on the CPU.
  1. every table row: the launcher reports the table's kernel; each of the m x n elements is finite and inside the derived bound; the
     floats in front of the output, columns n .. ldc - 1, rows >= m and the rows behind still hold the fill pattern, bit for bit; a launch
     whose residual aliases its output (fc2, post_proj) equals the non-aliased one bit for bit;
  2. tile-position invariance: equal input rows give bit-identical output rows wherever they sit - full tile or ragged last tile - in
     every precision, with and without GELU;
  3. forms that promise identical bits give them (the 128- and the 256-wide fp32-class tiles); forms that do not (gemm_f32_dma against
     gemm_f32_kernel, lin_x3 against the gemm_f16 build) are each inside the bound, and the switch demonstrably took effect;
  4. exact family: integer operands give the float64 result bit for bit in every precision and form - a dropped or doubled K-tile cannot
     hide inside a rounding bound;
  5. refusals (k % 32 with f16 operands, m <= 0, a null output) before anything is queued;
  6. the short-K dense GEMM through reid_cam_debias: cameras of 1 .. 5 rows, padded widths, fewer rows than columns.
Kernels are forced through Engine.debug_switch only (f32_conv, lin_x3, f16_lin_256, f16_cfg), restored in a finally.  Each row prints its
max error and worst error / bound; profiles/linear_gpu_tests.log is that output of one run."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as ref  # noqa: E402

pytestmark = [pytest.mark.gpu]
ERR_ARG = -1


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


def launch(eng, x, w, bias, res, precision, act=False, out_form=ref.OUT_F32, ldc=None, alias=False, x_fp32=False):
    """One harness call.  Checks the guard memory against the fill pattern and returns (form, bits [m, n or 2n]) - uint32 / uint16."""
    m, n = x.shape[0], w.shape[0]
    form, raw, front, ld = eng.debug_swin_linear(x, w, bias, res, precision, act, out_form, ldc, alias, x_fp32)
    bits, fill = (raw.view(np.uint32), np.uint32(0xffffffff)) if out_form == ref.OUT_F32 else (raw, np.uint16(0xffff))
    width = 2 * n if out_form == ref.OUT_PACKED else n
    assert bits.size == front + (m + 8) * ld and ld >= width
    assert (bits[:front] == fill).all(), "memory in front of the output was written"
    body = bits[front:].reshape(m + 8, ld)
    assert (body[m:] == fill).all(), "rows >= m were written: %s" % np.unique(np.nonzero(body[m:] != fill)[0])[:8]
    assert (body[:m, width:] == fill).all(), "columns n .. ldc - 1 were written"
    return form, np.ascontiguousarray(body[:m, :width])


def values(bits, out_form, n):
    if out_form == ref.OUT_F32:
        return bits.view(np.float32).astype(np.float64)
    f = bits.view(np.float16).astype(np.float64)
    return f if out_form == ref.OUT_F16 else f[:, :n] + f[:, n:] / 2048.0       # [yh | yl']: y = yh + yl' 2^-11


def check(got, want, bound, what):
    assert np.isfinite(got).all(), "%s: %d unwritten / non-finite outputs" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    ratio = err / np.maximum(bound, 1e-300)
    i = int(np.argmax(ratio))
    print("\nlinear %s: max |err| %.3e, worst err/bound %.4f over %d elements" % (what, err.max(), ratio.flat[i], err.size))
    assert ratio.flat[i] <= 1.0, "%s: element %s is %.3e off, bound %.3e" % (what, np.unravel_index(i, err.shape), err.flat[i], bound.flat[i])
    return float(ratio.flat[i])


def run_and_check(eng, x, w, bias, res, precision, act, out_form, ldc, x_fp32, what):
    form, bits = launch(eng, x, w, bias, res, precision, act, out_form, ldc, False, x_fp32)
    p = ref.oracle(x, w, bias, res, act, precision)
    b = ref.bound(p, precision, x.shape[1], act, out_form, split=precision == 2 and not x_fp32)
    check(values(bits, out_form, w.shape[0]), p.v, b, what)
    return form, bits


# ---------------------------------------------------------------------------------------------- 1. every launch form against float64
@pytest.mark.parametrize("row", ref.LINEAR_TABLE, ids=ref.row_id)
def test_every_table_row(eng, row):
    x, w, bias, res = ref.operands(row.m, row.n, row.k)
    bias = None if row.n == 3 * row.k else bias                 # to_qkv has no bias: the null col_shift
    res = res if row.res else None
    with switches(eng, **dict(row.switches)):
        form, bits = run_and_check(eng, x, w, bias, res, row.precision, row.act, row.out_form, row.ldc, row.x_fp32, ref.row_id(row))
        assert form == row.form, "launched %s" % ref.FORM_NAMES.get(form, form)
        if row.res == 2:
            form2, bits2 = launch(eng, x, w, bias, res, row.precision, row.act, row.out_form, row.ldc, True, row.x_fp32)
            assert form2 == row.form and np.array_equal(bits2, bits), "the in-place launch differs in %d elements" % (bits2 != bits).sum()


@pytest.mark.parametrize("m,n,k", [(129, 96, 36), (49, 5, 36)], ids=str)
def test_gemm_nt_with_k_off_the_tile(eng, m, n, k):
    """reid_gemm_nt, the public entry that reaches gemm_f32_kernel's K-tail guard with k % 32 != 0"""
    x, w, bias, _ = ref.operands(m, n, k)
    p = ref.oracle(x, w, bias)
    check(eng.gemm_nt(x, w, bias).astype(np.float64), p.v, ref.bound(p, 0, k), "gemm_nt %dx%dx%d" % (m, n, k))


# ---------------------------------------------------------------------------------------------- 2. tile-position invariance
# (precision, n, k, res, out_form, switches, m): m = 305 for the 128-row fp32 tiles, 561 for the 256-row f16 tiles - two full tiles + 49 rows
POSITION = [
    (0, 384, 96, 0, ref.OUT_F32, {}, 305), (0, 384, 96, 1, ref.OUT_F32, {}, 305), (0, 96, 384, 1, ref.OUT_F32, {}, 305),
    (0, 384, 96, 0, ref.OUT_F32, {"f32_conv": 0}, 305), (0, 384, 96, 1, ref.OUT_F32, {"f32_conv": 0}, 305),
    (1, 384, 96, 0, ref.OUT_F16, {}, 561), (1, 96, 384, 1, ref.OUT_F32, {}, 561), (1, 288, 96, 0, ref.OUT_F16, {}, 561),
    (2, 384, 96, 0, ref.OUT_PACKED, {}, 561), (2, 384, 384, 1, ref.OUT_F32, {}, 561), (2, 288, 96, 0, ref.OUT_PACKED, {}, 561),
    (2, 96, 96, 1, ref.OUT_F32, {}, 561), (2, 384, 96, 0, ref.OUT_PACKED, {"lin_x3": 0}, 561),
    (2, 768, 768, 1, ref.OUT_F32, {"lin_x3": 0}, 561), (2, 1536, 384, 0, ref.OUT_PACKED, {"lin_x3": 0}, 561),
]


@pytest.mark.parametrize("act", (0, 1), ids=("plain", "gelu"))
@pytest.mark.parametrize("case", POSITION, ids=lambda c: "p%d-%dx%d-%s-%s" % (c[0], c[1], c[2], ("nores", "res")[c[3]], "-".join("%s%d" % kv for kv in c[5].items()) or "default"))
def test_equal_rows_give_equal_bits_in_every_tile_position(eng, case, act):
    """Eight distinct rows repeated over m, the order rotated by one every eight rows so that each lands on every row of an MFMA
    accumulator block, in full tiles and in the ragged one: output rows of equal input rows are bit-identical (the kernel-level form of
    test_swin_embeddings_do_not_depend_on_the_pass_size; gemm_f16.hip: "a ragged last tile must give its rows what a full tile would")."""
    precision, n, k, has_res, out_form, sw, m = case
    x8, w, bias, res8 = ref.operands(8, n, k)
    idx = (np.arange(m) + np.arange(m) // 8) % 8
    tile = 128 if precision == 0 else 256
    assert set(idx[:tile]) == set(idx[m // tile * tile:]) == set(range(8))
    x, res = np.ascontiguousarray(x8[idx]), (np.ascontiguousarray(res8[idx]) if has_res else None)
    with switches(eng, **sw):
        _, bits = run_and_check(eng, x, w, bias, res, precision, act, out_form, None, False, "position p%d %dx%dx%d act%d" % (precision, m, n, k, act))
    bad = np.nonzero((bits != bits[:8][idx]).any(1))[0]
    assert bad.size == 0, "%d rows differ from their first copy, e.g. rows %s (tile rows %s)" % (bad.size, bad[:8], bad[:8] % tile)


# ---------------------------------------------------------------------------------------------- 3. forms against each other
@pytest.mark.parametrize("n,k", [(768, 768), (768, 3072)], ids=str)
@pytest.mark.parametrize("out_form", (ref.OUT_F32, ref.OUT_PACKED), ids=("f32res", "packed"))
def test_the_128_and_the_256_wide_fp32_class_tiles_are_bit_identical(eng, n, k, out_form):
    """gemm_f16.hip launch_any: "an output's K order is the same in both tiles: bit-identical results" """
    m = 305
    x, w, bias, res = ref.operands(m, n, k)
    res = res if out_form == ref.OUT_F32 else None
    got = {}
    for wide in (0, 1):
        with switches(eng, lin_x3=0, f16_lin_256=wide):
            form, got[wide] = launch(eng, x, w, bias, res, 2, False, out_form)
            assert form == (ref.LIN256 if wide else ref.LIN128) == ref.linear_form(2, m, n, k, out_form, {"lin_x3": 0, "f16_lin_256": wide})
    assert np.array_equal(got[0], got[1]), "%d elements differ" % (got[0] != got[1]).sum()


@pytest.mark.parametrize("act", (0, 1), ids=("plain", "gelu"))
def test_both_exact_fp32_kernels_are_inside_the_bound(eng, act):
    """gemm_f32_dma_kernel and gemm_f32_kernel are not promised identical for the Linear epilogue: each is held to the bound; whether they
    agree is printed."""
    x, w, bias, res = ref.operands(305, 384, 96)
    got = {}
    for dma in (1, 0):
        with switches(eng, f32_conv=dma):
            form, got[dma] = run_and_check(eng, x, w, bias, res, 0, act, ref.OUT_F32, None, False, "f32_conv=%d act%d" % (dma, act))
            assert form == (ref.DMA64 if dma else ref.F32_128)
    print("\nlinear gemm_f32_dma vs gemm_f32_kernel (act %d): %d of %d elements differ" % (act, (got[0] != got[1]).sum(), got[0].size))


@pytest.mark.parametrize("n,k,out_form,act", [(384, 384, ref.OUT_F32, 0), (1536, 384, ref.OUT_PACKED, 1)], ids=str)
def test_lin_x3_and_the_gemm_f16_build_are_both_inside_the_bound(eng, n, k, out_form, act):
    x, w, bias, res = ref.operands(305, n, k)
    res = res if out_form == ref.OUT_F32 else None
    got = {}
    for x3 in (1, 0):
        with switches(eng, lin_x3=x3):
            form, got[x3] = run_and_check(eng, x, w, bias, res, 2, act, out_form, None, False, "lin_x3=%d %dx%d" % (x3, n, k))
            assert form == (ref.X3 if x3 else ref.linear_form(2, 305, n, k, out_form, {"lin_x3": 0}))
    assert (got[0] != got[1]).any(), "lin_x3 = 0 changed nothing: the switch did not take effect"


# ---------------------------------------------------------------------------------------------- 4. exact family
# (precision, m, n, k, switches, form): k <= 384, every form such a K can reach
EXACT = [
    (0, 129, 288, 96, {}, ref.DMA64), (0, 305, 96, 384, {}, ref.DMA64), (0, 129, 96, 36, {}, ref.F32_128), (0, 33, 8, 4, {}, ref.F32_64),
    (0, 129, 288, 96, {"f32_conv": 0}, ref.F32_128), (0, 49, 96, 28, {}, ref.F32_128),
    (1, 257, 288, 96, {}, ref.LIN64), (1, 305, 384, 384, {}, ref.LIN128), (1, 257, 768, 384, {"f16_cfg": 256324}, ref.LIN256_BK32),
    (2, 305, 384, 384, {}, ref.X3), (2, 257, 384, 96, {}, ref.X3), (2, 257, 288, 96, {}, ref.LIN64), (2, 129, 96, 384, {}, ref.LIN128),
    (2, 305, 384, 384, {"lin_x3": 0}, ref.LIN128), (2, 257, 1536, 384, {"lin_x3": 0}, ref.LIN256),
    (2, 257, 768, 384, {"lin_x3": 0, "f16_cfg": 256324}, ref.LIN256_BK32),
]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "p%d-%s-%dx%dx%d" % (c[0], ref.FORM_NAMES[c[5]], c[1], c[2], c[3]))
def test_exact_family_is_bit_exact(eng, case):
    """Integer x, w in [-8, 8]: every product and partial sum is exact in fp32 and in the f16 hi parts, so fp32 output without GELU is the
    float64 result bit for bit in all three precisions - a dropped, doubled or misplaced K-tile or column shows as a whole number."""
    precision, m, n, k, sw, want_form = case
    x, w, bias, res = ref.exact_operands(m, n, k)
    with switches(eng, **sw):
        form, bits = launch(eng, x, w, bias, res, precision)
    assert form == want_form == ref.linear_form(precision, m, n, k, ref.OUT_F32, sw)
    want = ref.oracle(x, w, bias, res, False, precision).v.astype(np.float32)
    bad = np.nonzero(bits.view(np.float32) != want)
    assert bad[0].size == 0, "%d elements are not exact, first (%d, %d): %r against %r" % (
        bad[0].size, bad[0][0], bad[1][0], bits.view(np.float32)[bad][0], want[bad][0])


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(eng):
    from reid_amd import _ffi
    x, w, bias, _ = ref.operands(49, 96, 36)

    def refused(fn):
        with pytest.raises(_ffi.ReidHipError) as e:
            fn()
        assert e.value.status == ERR_ARG, e.value

    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 1, out_form=ref.OUT_F16))      # k % 32 != 0 with f16 operands
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 1))
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 2, out_form=ref.OUT_PACKED))
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 2))
    refused(lambda: eng.debug_swin_linear(x[:, :34], w[:, :34], bias, None, 0))            # k % 4 != 0 with fp32 operands
    x, w, bias, res = ref.operands(49, 96, 96)
    refused(lambda: eng.debug_swin_linear(x[:0], w, bias, None, 0))                        # m <= 0
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 0, out_form=ref.OUT_F16))      # a form the precision does not have
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 1, out_form=ref.OUT_PACKED))
    refused(lambda: eng.debug_swin_linear(x, w, bias, res, 1, out_form=ref.OUT_F16))       # f16 rows take no residual
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 0, ldc=100))                   # linear() writes rows of n
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 1, ldc=95, out_form=ref.OUT_F16))
    refused(lambda: eng.debug_swin_linear(x, w, bias, None, 0, alias=True))                # nothing to alias
    fn, form = _ffi.debug_lib().reid_debug_swin_linear, C.c_int(7)
    args = [C.c_void_p(a.ctypes.data) for a in (x, w, bias)] + [None, C.c_int(49), C.c_int(96), C.c_int(96)]
    buf = np.zeros(64 + 57 * 96, np.float32)
    for precision, out_form in ((0, 0), (1, 1), (2, 2)):                                   # the chosen form's output pointer is null
        out = [None, C.c_void_p(buf.ctypes.data)] if out_form == 0 else [C.c_void_p(buf.ctypes.data), None]
        assert fn(eng.h, *args, C.c_int(precision), C.c_int(0), C.c_int(out_form), C.c_int(96), *out, C.byref(form)) == ERR_ARG
    assert not buf.any()
    form, _ = launch(eng, x, w, bias, None, 0)                                             # and the context still works
    assert form == ref.DMA64


# ---------------------------------------------------------------------------------------------- 6. short-K dense GEMM through reid_cam_debias
def _unit_rows(rng, n, d):
    x = rng.normal(size=(n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


DEBIAS = {
    "d33-cameras-of-1-2-3-5-129": (33, (1, 2, 3, 5, 129)),
    "d1": (1, (3, 5)), "d2": (2, (2, 7, 4)), "d3": (3, (5, 9)), "d5": (5, (4, 6, 11)), "d7": (7, (3, 8)),     # dp padding
    "d130-rows-below-d": (130, (30, 30, 30)),
}


@pytest.mark.parametrize("name", sorted(DEBIAS))
def test_cam_debias_small_cameras(eng, name):
    """reid_cam_debias forms a camera's Gram matrix with K = its row count padded to 4: cameras of 1 .. 28 rows are the only callers of
    gemm_f32_kernel<A_DENSE, E_BIAS> with K < 32.  Against oracle/postproc.diminish_camera_bias at the project's atol; a single-row
    camera is 0 / 0 in the reference and NaN here, exactly there."""
    from oracle import postproc
    d, sizes = DEBIAS[name]
    la = 0.05
    rng = np.random.default_rng(sorted(DEBIAS).index(name) + 500)
    x = _unit_rows(rng, sum(sizes), d)
    cams = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    for c, nc in enumerate(sizes):      # precondition, in float64: well-conditioned inputs only (ill-conditioned ones are out of scope)
        cur = x[cams == c].astype(np.float64)
        assert cur.shape[0] == nc
        A = cur.T @ cur + nc * la * np.eye(d)
        assert np.abs(A).sum(1).max() / (nc * la) < 100
    with np.errstate(invalid="ignore", divide="ignore"):
        want = postproc.diminish_camera_bias(x, cams, la)
    got = eng.cam_debias(x, cams, la)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN masks differ: rows %s" % np.nonzero(np.isnan(got).any(1) != np.isnan(want).any(1))[0]
    assert np.isnan(want[cams == sizes.index(1)]).all() if 1 in sizes else np.isfinite(want).all()
    print("\nlinear cam_debias %s: max |err| %.3e" % (name, np.nanmax(np.abs(got - want))))
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-5)
