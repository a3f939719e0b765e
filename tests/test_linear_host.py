"""CPU checks of tests/linear_ref.py, the reference side of tests/test_gpu_linear.py: the dispatch predicates against the case table, the
float64 oracle, the shape of the bound, and that the table reaches every launch form, epilogue variant and edge the Linear layers have."""
import math
import os
import re
import sys

import numpy as np
import pytest

from reid_amd import _ffi
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = ref.LINEAR_TABLE


def _rows(precision=None, form=None):
    return [r for r in TABLE if (precision is None or r.precision == precision) and (form is None or r.form == form)]


# ---------------------------------------------------------------------------------------------- dispatch
@pytest.mark.parametrize("row", TABLE, ids=ref.row_id)
def test_linear_form_agrees_with_the_table(row):
    assert ref.linear_form(row.precision, row.m, row.n, row.k, row.out_form, dict(row.switches), row.x_fp32) == row.form
    assert row.ldc >= row.n and (row.precision == 1 or row.ldc == row.n)
    assert row.out_form == ref.OUT_F32 or (row.out_form == row.precision and not row.res and not row.x_fp32)


def test_table_rows_are_distinct_and_ids_unique():
    assert len(set(TABLE)) == len(TABLE)
    assert len({ref.row_id(r) for r in TABLE}) == len(TABLE)


def test_linear_form_refusals_and_switches():
    with pytest.raises(ValueError):
        ref.linear_form(1, 49, 96, 36)                 # launch_gemm_f16: K % 32
    with pytest.raises(ValueError):
        ref.linear_form(0, 49, 96, 6)                  # launch_gemm_f32: K % 4
    with pytest.raises(ValueError):
        ref.linear_form(1, 49, 96, 96, switches={"f16_cfg": 64642})   # no LIN build of that tile outside experiment builds
    # an override whose width does not divide N falls back to the heuristic (launch_any)
    assert ref.linear_form(1, 49, 288, 96, switches={"f16_cfg": 256324}) == ref.LIN64
    # the 256-wide tile needs 3 k >= 1152, 3 k % 64 == 0 and n % 256 == 0
    assert ref.linear_form(2, 49, 768, 352, switches={"lin_x3": 0}) == ref.LIN128          # 3 k = 1056
    assert ref.linear_form(2, 49, 768, 416, switches={"lin_x3": 0}) == ref.LIN128          # 3 k = 1248, not a multiple of 64
    assert ref.linear_form(2, 49, 1152, 768, switches={"lin_x3": 0}) == ref.LIN128         # 1152 % 256 != 0
    assert ref.linear_form(1, 49, 768, 768) == ref.LIN128                                  # fp16 storage never takes it
    # the batch never moves a Linear's tile
    for m in (1, 49, 305, 100000):
        assert ref.linear_form(2, m, 768, 768) == ref.X3 and ref.linear_form(1, m, 384, 96) == ref.LIN128
    assert ref.attn_ldq(1, 96) == 320 and ref.attn_ldq(1, 192) == 576 and ref.attn_ldq(2, 96) == 288


def test_predicates_restate_the_sources():
    """The constants the predicates lean on are still the sources' (a changed heuristic must change linear_form with it)."""
    csrc = os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc")
    f16 = open(os.path.join(csrc, "gemm_f16.hip")).read()
    assert "if (p.lin && ctx->f16_lin_256 && p.split_terms && p.N % 256 == 0 && k64 && p.K >= 1152) bn = 256;" in f16
    assert "else if (p.lin) cfg = bn == 256 ? 256642 : bn * 1000 + 323;" in f16
    assert "ctx->conv_form = STAG * 1000000 + BN * 1000 + BK * 10 + NST;" in f16
    dma = open(os.path.join(csrc, "gemm_f32_dma.hip")).read()
    assert "if (EPI == E_BIAS || p.N <= 64 || cost64 < cost128) {" in dma and "ctx->conv_form = %d;" % ref.DMA64 in dma
    assert "p.K % 32 == 0 && p.lda % 4 == 0 && p.ldb % 4 == 0" in dma
    f32 = open(os.path.join(csrc, "gemm_f32.hip")).read()
    assert "ctx->conv_form = p.N <= 64 ? %d : %d;" % (ref.F32_64, ref.F32_128) in f32
    assert "if (ctx->f32_conv == 1 && gemm_f32_dma_supported(amode, epi, p)) return launch_gemm_f32_dma" in f32
    x3 = open(os.path.join(csrc, "conv3x3_x3.hip")).read()
    assert "ctx->conv_form = %d;" % ref.X3 in x3
    assert "p.K % 96 == 0 && p.N % 128 == 0 && p.n_real == p.N" in x3


def test_harness_is_declared_exported_and_goes_through_the_forward_functions():
    hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    assert "int reid_debug_swin_linear(" in hdr and "reid_debug_swin_linear" in _ffi.DEBUG_EXPORTS
    assert hasattr(_ffi.debug_lib(), "reid_debug_swin_linear") and hasattr(Engine, "debug_swin_linear")
    for code in (ref.DMA64, ref.F32_64, ref.F32_128, ref.X3, ref.LIN64, ref.LIN128, ref.LIN256, ref.LIN256_BK32):
        assert str(code) in hdr, code
    csrc = os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc")
    internal = open(os.path.join(csrc, "reid_internal.h")).read()
    assert "int swin_linear_for_test(" in internal
    dbg = open(os.path.join(csrc, "debug.hip")).read()
    body = dbg[dbg.index('extern "C" int reid_debug_swin_linear('):]
    body = body[:body.index("\n}\n")]
    assert "swin_linear_for_test(" in body and not re.search(r"launch_gemm_f(16|32)\(|launch_lin_x3\(", body)
    swin = open(os.path.join(csrc, "swin.hip")).read()
    wrap = swin[swin.index("int swin_linear_for_test("):]
    wrap = wrap[:wrap.index("\n}\n")]
    assert "return linear16(ctx," in wrap and "return linear(ctx," in wrap


# ---------------------------------------------------------------------------------------------- oracle
def test_oracle_equals_a_triple_loop():
    x, w, bias, res = ref.operands(3, 5, 4)
    p = ref.oracle(x, w, bias, res, act=True)
    for i in range(3):
        for j in range(5):
            acc = sum(float(x[i, t]) * float(w[j, t]) for t in range(4))
            A = sum(abs(float(x[i, t])) * abs(float(w[j, t])) for t in range(4))
            h = acc + float(bias[j])
            v = 0.5 * h * (1.0 + math.erf(h / math.sqrt(2.0))) + float(res[i, j])
            assert abs(p.acc[i, j] - acc) <= 1e-15 * A and abs(p.A[i, j] - A) <= 1e-15 * A
            assert abs(p.v[i, j] - v) <= 1e-15 * (A + abs(v) + 1)


def test_oracle_is_exact_on_integers():
    x, w, bias, res = ref.exact_operands(37, 19, 384)
    p = ref.oracle(x, w, bias, res)
    want = x.astype(np.int64) @ w.astype(np.int64).T + bias.astype(np.int64) + res.astype(np.int64)
    assert np.array_equal(p.v, want.astype(np.float64))
    assert np.abs(p.A).max() <= 64 * 384 < 2 ** 24 and np.abs(want).max() < 2 ** 24
    p1 = ref.oracle(x, w, bias, res, precision=1)           # integers up to 8 are f16 values
    assert np.array_equal(p1.v, p.v)


def test_oracle_precision_1_runs_on_the_rounded_operands():
    x, w, bias, _ = ref.operands(9, 7, 32)
    p = ref.oracle(x, w, bias, precision=1)
    assert np.array_equal(p.acc, ref.f16r(x).astype(np.float64) @ ref.f16r(w).astype(np.float64).T)
    assert not np.array_equal(p.acc, ref.oracle(x, w, bias).acc)


# ---------------------------------------------------------------------------------------------- bound
def test_bound_is_monotone_and_ordered():
    x, w, bias, res = ref.operands(16, 24, 96)
    p = ref.oracle(x, w, bias, res, act=True)
    for prec in (0, 1, 2):
        b = ref.bound(p, prec, 96, act=True)
        assert (b > 0).all()
        assert (ref.bound(p, prec, 192, act=True) > b).all()                       # K
        assert (ref.bound(p._replace(A=2 * p.A), prec, 96, act=True) > b).all()     # A
        plain = ref.oracle(x, w, bias, res)
        assert (ref.bound(p._replace(g=plain.g, v=plain.v), prec, 96, act=True) > ref.bound(plain, prec, 96)).all()   # GELU costs
    assert (ref.bound(p, 2, 96) > ref.bound(p, 0, 96)).all()                        # the split contraction
    assert (ref.bound(p, 1, 96, out_form=ref.OUT_F16) > ref.bound(p, 1, 96)).all()
    assert (ref.bound(p, 2, 96, out_form=ref.OUT_PACKED) > ref.bound(p, 2, 96)).all()


def test_gelu_constants():
    h = np.linspace(-12.0, 12.0, 480001)
    erf = np.array([math.erf(t / math.sqrt(2.0)) for t in h])
    d = 0.5 * (1.0 + erf) + h * np.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)      # GELU'
    assert 1.128 < np.abs(d).max() < ref.GELU_LIP
    # Abramowitz-Stegun 7.1.28 with the coefficients of csrc/lin_math.h, in float64, against math.erf
    src = open(os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc", "lin_math.h")).read()
    body = src[src.index("float gelu_f16_storage(float v)"):src.index("return fmaf(h, copysignf(erfz, v), h);")]
    coef = [float(c) for c in re.findall(r"(\d\.\d+)f", body)]
    assert len(coef) == 10 and coef[0] == 0.70710678118654752440 and coef[7] == coef[8] == 1.0 and coef[9] == 0.5, coef
    z = np.linspace(0.0, 9.0, 90001)
    q = np.full_like(z, coef[1])
    for c in coef[2:8]:
        q = q * z + c
    approx = 1.0 - q ** -16.0
    assert np.abs(approx - np.array([math.erf(t) for t in z])).max() <= ref.AS_ERR
    assert body.count("fmaf(") == 6 and body.count("q = q * q;") == 4 and "__builtin_amdgcn_rcpf(q)" in body
    assert ref.AS_CHAIN == (((6 * 2 + 1) * 2 + 1) * 2 + 1) * 2 + 1 + 2           # six fmaf, four squarings, one rcp of 1 ulp
    assert max(t * 2 / math.sqrt(math.pi) * math.exp(-t * t) for t in z) < 0.49  # z erf'(z): a 2u relative z is < 1u of erf


# ---------------------------------------------------------------------------------------------- coverage of the table
def test_every_required_form_is_in_the_table():
    for prec, forms in ref.REQUIRED_FORMS.items():
        for form in forms:
            assert _rows(prec, form), (prec, ref.FORM_NAMES[form])
    assert all(r.form in ref.FORM_NAMES for r in TABLE)
    assert {r.m for r in TABLE} >= {1, 49, 127, 128, 129, 255, 256, 257, 305}
    shapes = {(288, 96), (96, 96), (384, 96), (96, 384), (576, 192), (1152, 384), (384, 384), (1536, 384), (384, 1536), (768, 768), (3072, 768),
              (768, 3072)}
    for prec in (0, 1, 2):
        have = {(r.n, r.k) for r in _rows(prec)}
        assert shapes <= have, (prec, shapes - have)
    assert {(751, 96), (751, 512), (5, 96)} <= {(r.n, r.k) for r in _rows(0)}


def test_precision_0_rows_cover_every_epilogue_variant_and_edge():
    dma = _rows(0, ref.DMA64)
    lean = {(r.act, bool(r.res)) for r in dma if "lean" in ref.epilogue_paths(r.form, r.m, r.n, r.out_form)}
    assert lean == {(0, False), (0, True), (1, False), (1, True)}
    general = [r for r in dma if r.m < 128]
    assert {(r.act, bool(r.res)) for r in general} >= {(0, False), (0, True), (1, False)}
    assert {r.m for r in dma if r.m > 128 and r.m % 128} >= {129, 305}                     # the ragged tail behind full tiles
    assert any(r.res == 2 for r in dma if r.m >= 128) and any(r.res == 2 for r in dma if r.m % 128)
    no_dma = [r for r in _rows(0) if dict(r.switches).get("f32_conv") == 0]
    assert {r.form for r in no_dma} == {ref.F32_64, ref.F32_128}
    assert {r.form for r in _rows(0) if r.k == 36} == {ref.F32_64, ref.F32_128}
    assert {(r.n, r.k) for r in _rows(0) if r.k < 32} >= {(n, k) for n in (8, 96) for k in (4, 8, 28)}
    assert any(r.n == 751 and r.ldc % 2 == 1 and r.m >= 128 for r in dma) and any(r.n == 751 and r.m < 128 for r in dma)
    assert [r for r in _rows(2) if r.x_fp32 and r.form == ref.DMA64]


def test_precision_1_rows_cover_every_form_and_output():
    assert {r.n for r in _rows(1, ref.LIN64)} >= {288, 192, 576}
    assert {r.n for r in _rows(1, ref.LIN128)} >= {96, 384, 768}
    f16 = [r for r in _rows(1) if r.out_form == ref.OUT_F16]
    assert any(r.ldc == ref.attn_ldq(1, 96) == 320 and r.n == 288 for r in f16) and any(r.ldc == r.n for r in f16)
    assert any(r.act for r in f16)
    f32 = [r for r in _rows(1) if r.out_form == ref.OUT_F32]
    assert f32 and all(r.res for r in f32) and any(r.res == 2 for r in f32)
    for form in (ref.LIN64, ref.LIN128):
        paths = set().union(*(ref.epilogue_paths(r.form, r.m, r.n, r.out_form) for r in _rows(1, form)))
        assert paths == {"staged", "stream", "general"}, (form, paths)
    assert all(dict(r.switches).get("f16_cfg") == 256324 for r in TABLE if r.form == ref.LIN256_BK32)


def test_precision_2_rows_cover_every_form_and_output():
    x3 = _rows(2, ref.X3)
    assert {r.n for r in x3} >= {384, 768, 1152, 1536, 3072}
    assert any(r.out_form == ref.OUT_PACKED and r.act for r in x3) and any(r.out_form == ref.OUT_PACKED and not r.act for r in x3)
    assert any(r.out_form == ref.OUT_F32 and r.res == 2 for r in x3) and any(r.out_form == ref.OUT_F32 and r.res == 1 for r in x3)
    assert {r.n for r in _rows(2, ref.LIN64)} >= {288, 192, 576}
    lin128 = _rows(2, ref.LIN128)
    assert any(r.n == 96 for r in lin128) and any(r.n % 128 == 0 and dict(r.switches).get("lin_x3") == 0 for r in lin128)
    lin256 = _rows(2, ref.LIN256)
    assert {(r.n, r.k) for r in lin256} >= {(768, 768), (3072, 768), (768, 3072)}
    assert all(dict(r.switches).get("lin_x3") == 0 and r.n % 256 == 0 and 3 * r.k >= 1152 and 3 * r.k % 64 == 0 for r in lin256)
    for form in (ref.LIN64, ref.LIN128, ref.LIN256):
        paths = set().union(*(ref.epilogue_paths(r.form, r.m, r.n, r.out_form) for r in _rows(2, form)))
        assert paths >= {"staged", "general"} and ("stream" in paths or form == ref.LIN256), (form, paths)
