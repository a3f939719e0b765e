"""The fp16-storage trunk's convolutions (precision 1) layer by layer, each launch form against a float64 oracle (debug harnesses
reid_debug_conv_layer_f16 and reid_debug_conv_c64_se; csrc/conv3x3_f16.hip, csrc/gemm_f16.hip, csrc/conv3x3_c64_f16.hip).

Every launch goes through conv_gemm16(A16_IM2COL, ...), the call the forward makes, or through launch_conv3x3_c64_f16, with the context's
switches.  The launchers report the launch they made (`form`, include/reid_hip_debug.h): the tile configuration BN*1000 + BK*10 + NST of
the implicit GEMM, BN*10 + split K of the LDS-halo kernel, 1 / 2 for the layer-1 kernel without / with the fused SE tail.  Each case
compares it with a literal.  Run on an MI355X: pytest -m gpu tests/test_gpu_conv_f16.py.

Operands.  Normal-distributed values rounded to f16 on the host (weights / sqrt(K) first), handed over as bits: the kernel and the oracle
see the same numbers.  Residual f16; scale in +-[0.5, 1.5] (a fifth of the columns negative), shift N(0, 1/2).  Image 0 carries a
constant top row (3) and left column (-2), so that a shifted tap shows.

Oracle.  test_gpu_conv.py's: a float64 convolution of those values (acc) and A = sum |x||w|, then v = acc scale + shift (+ res), ReLU.
Launches above 4096 rows are checked on sample_rows (whole first / last / a seeded 128-row group, first and last rows of every 256-row
tile, the borders of the first and last image, 64 seeded rows) plus the middle group; every output is checked densely for the NaN fill.

Error bound per element (u = 2^-24, H = 2^-11 the f16 half-ulp, 2^-25 the same below f16's normal range, SAFETY = 2: as chosen in
test_gpu_conv.py and test_gpu_tail.py).  Operands are exact, products of two f16 are exact in fp32, sums are fp32:
  GEMM and halo kernels:  e32 = SAFETY (|scale| K u A + 4u (|acc scale| + |shift| + |res|))     (accumulation over K = R S Cin, in any split-K
                          order; the epilogue's multiply and adds), ReLU is 1-Lipschitz;  bound = e32 + H (|v| + e32) + 2^-25.
  their stats (sums of the fp32 values before the f16 rounding, gemm_f16.hip pass1 / conv3x3_f16.hip pass1, per 128 rows):
                          sum e32 + SAFETY 128u sum|v|;  sum (2|v| e32 + e32^2) + SAFETY 129u sum v^2.
  layer-1 kernel (c64):   the weights arrive with the BN scale folded in, w16 = f16(w32 scale32) (what scale_rows_f16_kernel makes; the test
                          forms them on the host, so scale = 1 below).  The accumulator is rounded to f16 BEFORE shift and residual:
                          ea = SAFETY K u A,  e16 = ea + H (|acc| + ea) + 2^-25.  The raw form stores that value: bound = e16, and its
                          stats sum the f16 value.  Otherwise e32 = e16 + SAFETY 4u (|acc| + |shift| + |res|), bound = e32 + H (|v| + e32)
                          + 2^-25, and the stats sum the fp32 value before the last rounding (conv3x3_c64_f16.hip:186-191), per image:
                          sum e + SAFETY 2048u sum|v|;  sum (2|v| e + e^2) + SAFETY 2049u sum v^2  (e = e16 or e32).
  fused SE tail:          y = the value above, rounded to f16 into the scratch image: e_y = e32 + H (|y| + e32) + 2^-25.  pooled = s1 / 2048 with
                          d_pooled = (the c64 bound of s1) / 2048 + u |pooled|; the gate by test_gpu_tail.py's SE model with d_pooled carried
                          into the hidden units: d_h = 64u sum|w1||pooled| + sum|w1| d_pooled, d_g = SAFETY (1/4 (8u sum|w2||h| + sum|w2| d_h)
                          + 4u g).  out32 = relu(g y16 + sc): |y| d_g + (g + d_g) e_y + SAFETY 2u (|g y| + |sc|) =: e_o, and
                          bound = e_o + H (|out| + e_o) + 2^-25.  (A shorter model, g (H|y| + 2^-25) in place of (g + d_g) e_y, leaves
                          out e32: y's own accumulation and first-rounding error passes through the gate too.  It is printed, not asserted.)

Forms.  Halo kernel (launch_geom's cost rule; chunks = Cin / 64 is 1, 2, 4 or 8 at the trunk's shapes):
  l2 (2 chunks)   n = 1 -> 642, 40 -> 641, 65 -> 1281          l3 (4)   n = 2, 3 -> 644, 40 -> 642, 100 -> 641, 130, 131 -> 1281
  l4a (4)         n = 2, 3 -> 644, 67 -> 1281                  l4 (8)   n = 3, 16 -> 644, 24 -> 642, 40 -> 641, 66, 67 -> 1281
  l1 (1 chunk) under f16_halo = 2 only (geometry <32,1>): n = 2, 40 -> 641.
  Not reachable in this mode, by the rule itself: split K 3 (no chunk count is divisible by 3) and the 128-wide split-K forms of
  f16_wide_splitk (1282 .. 1284 need 12 or more chunks): both belong to the fp32-class build, whose virtual Cin is three times as large.
  The unsplit 128-wide form "at exactly 128 tiles" (l3 n = 128, l2 / l4 n = 64): its cost 1.3 x chunks x 9 + 0.0005 is twice the 64-wide
  form's 0.65 x chunks x 9 - 0.0019 at one round each (256 tiles), so 641 wins at every batch; the l3 n = 128 case records 641.
Implicit GEMM (launch_any): l1 n = 2 -> 64642; l2s, l2d -> 128323; l3s, l3d n = 2, 3 -> 64642, 128, 129 -> 128642, 384 -> 256642; l4d n = 2, 3 ->
  64642, 64 -> 128642, 192 -> 256642; the stride-1 layers under f16_halo = 0: l2 -> 128323, l3, l4 n = 2 -> 64642; Cin = 96 (BK = 32 builds): 16 x 8,
  256 channels out, n = 3 -> 64323, 512 out, n = 192 -> 256324.  Every build of the product library's conv switch is named here.
Layer-1 kernel: 1 (plain), 2 (fused SE).

Recorded on an MI355X, max err / bound per family (not asserted):
  family            values   sum     sum of squares
  halo kernel       0.72     <0.001  <0.001       (K = 576 .. 4608: K u A leads, the f16 half-ulp is 0.1 .. 0.7 of the bound)
  implicit GEMM     0.97     0.003   0.003        (the 1x1 convolutions, K = 64 .. 256: the bound is all but the half-ulp, and a tie is met)
  layer-1 kernel    0.71     0.008   0.026
  fused SE tail     0.67                          (against the shorter model, without e32 through the gate: 4.7 .. 6.1)
The stats bounds sum the worst-case element errors of 128 (2048) rows, whose signs are random on the device: hence the small ratios.
Broken on purpose in a scratch copy of conv3x3_f16.hip, each made cases fail: a halo pixel (row 0, last column) read as padding - every
halo case; the reduction of one tile leaving out the last split-K slice - every split-K halo case (values out of bound); the arrival counter
not reset by the last block - every split-K case from its second launch on (outputs left as NaN), test_split_k_state included.
"""
import numpy as np
import pytest

import test_gpu_conv as tc
from test_gpu_conv import LAYERS, conv_oracle, epilogue, sample_rows
from reid_amd import _ffi, synth, weights

gpu = pytest.mark.gpu

U = tc.U
H = 2.0 ** -11
H_ABS = 2.0 ** -25
SAFETY = tc.SAFETY

SWITCHES = ("f16_halo", "f16_cfg", "f16_split_k", "f16_wide_splitk", "f16_c64")
EXTRA_LAYERS = {"c96a": (16, 8, 96, 256, 3, 1, 1), "c96b": (16, 8, 96, 512, 3, 1, 1)}     # Cin not divisible by 64: the BK = 32 builds
SHAPES = dict(LAYERS, **EXTRA_LAYERS)


# ----------------------------------------------------------------------------- operands and bounds
def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def out_shape(layer):
    h, w, cin, cout, r, stride, pad = SHAPES[layer]
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1


def operands(layer, n, seed):
    """x, w, residual as float16; scale, shift fp32."""
    h, w, cin, cout, r, stride, pad = SHAPES[layer]
    ho, wo = out_shape(layer)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, cin), np.float32).astype(np.float16)
    x[0, 0, :, :] = 3.0
    x[0, :, 0, :] = -2.0
    wt = f16(rng.standard_normal((cout, r, r, cin), np.float32) / np.float32(np.sqrt(r * r * cin)))
    scale = (rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.2, -1.0, 1.0)).astype(np.float32)
    shift = rng.normal(0, 0.5, cout).astype(np.float32)
    res = rng.standard_normal((n, ho, wo, cout), np.float32).astype(np.float16)
    return x, wt, scale, shift, res


def rows_to_check(layer, n, seed):
    """sample_rows plus whole 128-row groups (first, middle, last) for the stats."""
    ho, wo = out_shape(layer)
    m = n * ho * wo
    rows = sample_rows(n, ho, wo, seed)
    groups = np.array(sorted({0, m // 128 // 2, m // 128 - 1}))
    rows = np.unique(np.concatenate([rows] + [np.arange(g * 128, g * 128 + 128) for g in groups]))
    return rows, groups


def oracle_rows(x, wt, stride, pad, rows, hw, chunk=32):
    """conv_oracle on `rows`, a chunk of images at a time (a convolution does not cross images): the float64 copies stay small."""
    img = rows // hw
    acc = np.empty((len(rows), wt.shape[0]))
    ab = np.empty_like(acc)
    for i0 in range(int(img[0]) // chunk * chunk, int(img[-1]) + 1, chunk):
        sel = np.nonzero((img >= i0) & (img < i0 + chunk))[0]
        if len(sel):
            acc[sel], ab[sel] = conv_oracle(x[i0:i0 + chunk].astype(np.float64), wt, stride, pad, rows[sel] - i0 * hw)
    return acc, ab


def e32_bound(acc, ab, k, scale=None, shift=None, res=None):
    sc = 1.0 if scale is None else np.abs(np.asarray(scale, np.float64))
    sh = 0.0 if shift is None else np.abs(np.asarray(shift, np.float64))
    rr = 0.0 if res is None else np.abs(res)
    return SAFETY * (sc * k * U * ab + 4 * U * (np.abs(acc * sc) + sh + rr))


def rounded(v, e):
    """Bound of f16(v') for |v' - v| <= e."""
    return e + H * (np.abs(v) + e) + H_ABS


def ratio(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: non-finite (unwritten?) output" % what
    err = np.abs(got - want)
    q = err / np.maximum(bound, 1e-300)
    worst = np.unravel_index(np.argmax(q), q.shape)
    print("%s: max err / bound %.3f" % (what, q[worst]))
    assert (err <= bound).all(), "%s: at %s got %r, float64 %r, bound %g (err / bound %.3f)" % (
        what, worst, got[worst], want[worst], bound[worst], q[worst])
    return float(q[worst])


def group_stats_check(stats, groups, pos, v, e, nsum, what):
    """stats [groups, cout, 2] of `nsum`-row groups against the float64 sums of the oracle rows pos[g]."""
    for g in groups:
        vg, eg = v[pos[g]], e[pos[g]]
        assert len(vg) == nsum
        b1 = eg.sum(0) + SAFETY * nsum * U * np.abs(vg).sum(0)
        b2 = (eg * (2 * np.abs(vg) + eg)).sum(0) + SAFETY * (nsum + 1) * U * (vg * vg).sum(0)
        ratio(stats[g, :, 0], vg.sum(0), b1, "%s group %d sum" % (what, g))
        ratio(stats[g, :, 1], (vg * vg).sum(0), b2, "%s group %d sum of squares" % (what, g))


EPILOGUES = (("raw+stats", False, False, False, True),          # IBN conv1
             ("bn+relu", True, False, True, False),             # layer 4's conv1
             ("bn+res+relu+stats", True, True, True, True),     # conv2
             ("bn", True, False, False, False))                 # conv2 of a block with a downsample, and the downsample


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    sd = synth.seres18_state_dict(0)              # a loaded checkpoint: the zero page of the convolutions' padding
    blob, manifest, _ = weights.pack_seres18(sd)
    e.load_seres18(blob, manifest)
    return e


@pytest.fixture(scope="module")
def defaults(eng):
    return {k: eng.debug_switch(k) for k in SWITCHES}


def run(eng, defaults, layer, x, wt, switches=None, **kw):
    h, w, cin, cout, r, stride, pad = SHAPES[layer]
    try:
        for k, v in (switches or {}).items():
            eng.debug_switch(k, v)
        return eng.debug_conv_layer_f16(x, wt, stride, pad, **kw)
    finally:
        for k in (switches or {}):
            eng.debug_switch(k, defaults[k])


def check_layer(eng, defaults, layer, n, form, switches=None, seed=0):
    """All four epilogues of one (layer, batch) against the oracle, `form` against the literal; returns {epilogue: out}."""
    h, w, cin, cout, r, stride, pad = SHAPES[layer]
    k = r * r * cin
    x, wt, sc, sh, res = operands(layer, n, seed or (100 * n + len(layer) + cin))
    rows, groups = rows_to_check(layer, n, n)
    acc, ab = oracle_rows(x, wt, stride, pad, rows, out_shape(layer)[0] * out_shape(layer)[1])
    rr = res.reshape(-1, cout)[rows].astype(np.float64)
    index = {q: i for i, q in enumerate(rows)}
    pos = {g: [index[q] for q in range(g * 128, g * 128 + 128)] for g in groups}
    outs = {}
    for name, bn, with_res, relu, stats in EPILOGUES:
        what = "%s n=%d %s %s" % (layer, n, switches or "", name)
        out, st, got_form = run(eng, defaults, layer, x, wt, switches, scale=sc if bn else None, shift=sh if bn else None,
                                residual=res if with_res else None, relu=relu, stats=stats)
        assert got_form == form, "%s: launch form %d, expected %d" % (what, got_form, form)
        assert np.isfinite(out.astype(np.float32)).all(), "%s: an output was not written" % what
        v = epilogue(acc, sc if bn else None, sh if bn else None, rr if with_res else None, relu)
        e = e32_bound(acc, ab, k, sc if bn else None, sh if bn else None, rr if with_res else None)
        ratio(out.reshape(-1, cout)[rows], v, rounded(v, e), what)
        if stats:
            assert st.shape == (n * out_shape(layer)[0] * out_shape(layer)[1] // 128, cout, 2)
            assert np.isfinite(st).all(), "%s: a stats group was not written" % what
            group_stats_check(st, groups, pos, v, e, 128, what)
        outs[name] = (out, st)
    return outs


# ----------------------------------------------------------------------------- CPU: the model's pieces
def test_rounding_model_holds_for_numpy_f16():
    """|f16(v) - v| <= H |v| + 2^-25 over normal and subnormal values (the model every bound here ends with)."""
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(size=20000) * 10.0 ** rng.uniform(-9, 4, 20000), [0.0, 2.0 ** -24, 2.0 ** -25, 65504.0, 2.0 ** -14]])
    assert (np.abs(v.astype(np.float16).astype(np.float64) - v) <= H * np.abs(v) + H_ABS).all()


def test_operands_are_f16_and_carry_the_border_marks():
    x, wt, sc, sh, res = operands("l3", 2, 1)
    assert x.dtype == wt.dtype == res.dtype == np.float16 and sc.dtype == sh.dtype == np.float32
    assert (x[0, 0, 1:] == 3).all() and (x[0, 1:, 0] == -2).all() and (sc < 0).any() and (sc > 0).any()
    assert (np.abs(sc) >= 0.5).all() and (np.abs(sc) <= 1.5).all()


# ----------------------------------------------------------------------------- halo kernel
HALO_CASES = [
    ("l2", 1, 642, None), ("l2", 40, 641, None), ("l2", 65, 1281, None),
    ("l3", 2, 644, None), ("l3", 3, 644, None), ("l3", 40, 642, None), ("l3", 100, 641, None), ("l3", 128, 641, None),
    ("l3", 130, 1281, None), ("l3", 131, 1281, None),
    ("l4a", 2, 644, None), ("l4a", 3, 644, None), ("l4a", 67, 1281, None),
    ("l4", 3, 644, None), ("l4", 16, 644, None), ("l4", 24, 642, None), ("l4", 40, 641, None), ("l4", 66, 1281, None), ("l4", 67, 1281, None),
    ("l1", 2, 641, {"f16_halo": 2}), ("l1", 40, 641, {"f16_halo": 2}),
]


@gpu
@pytest.mark.parametrize("layer,n,form,sw", HALO_CASES, ids=["%s-n%d" % c[:2] for c in HALO_CASES])
def test_halo_kernel(eng, defaults, layer, n, form, sw):
    """launch_conv3x3_f16 at the default switches (layer 1: f16_halo = 2): the four epilogues of the forward, values and stats."""
    check_layer(eng, defaults, layer, n, form, sw)


SPLITK_CASES = [("l2", 1, 642, ("l3", 2, 644)), ("l3", 2, 644, ("l2", 1, 642)), ("l3", 40, 642, ("l4", 16, 644)),
                ("l4", 16, 644, ("l3", 40, 642)), ("l4", 24, 642, ("l3", 3, 644)), ("l4a", 3, 644, ("l2", 1, 642))]


@gpu
@pytest.mark.parametrize("layer,n,form,other", SPLITK_CASES, ids=["%s-n%d" % c[:2] for c in SPLITK_CASES])
def test_split_k_state(eng, defaults, layer, n, form, other):
    """Three repeats of a split-K launch with a split-K launch of another layer and another split between them: bit-identical (the
    arrival counters are shared and reset by the last block to arrive; the workspace is shared too).  With f16_split_k = 0 the same
    operands are unsplit and within the bound."""
    h, w, cin, cout, r, stride, pad = SHAPES[layer]
    x, wt, sc, sh, res = operands(layer, n, 500 + n)
    ox, ow, osc, osh, ores = operands(other[0], other[1], 600 + n)
    kw = dict(scale=sc, shift=sh, residual=res, relu=True, stats=True)
    outs = []
    for i in range(3):
        o, st, f = run(eng, defaults, layer, x, wt, **kw)
        assert f == form
        outs.append((o.view(np.uint16), st))
        oo, ost, of = run(eng, defaults, other[0], ox, ow, scale=osc, shift=osh, residual=ores, relu=True, stats=True)
        assert of == other[2] and np.isfinite(oo.astype(np.float32)).all() and np.isfinite(ost).all()
    for o, st in outs[1:]:
        np.testing.assert_array_equal(o, outs[0][0])
        np.testing.assert_array_equal(st, outs[0][1])
    check_layer(eng, defaults, layer, n, 641, {"f16_split_k": 0}, seed=500 + n)


# ----------------------------------------------------------------------------- implicit GEMM
GEMM_CASES = [
    ("l1", 2, 64642, None), ("l2s", 1, 128323, None), ("l2s", 9, 128323, None), ("l2d", 1, 128323, None), ("l2d", 9, 128323, None),
    ("l3s", 2, 64642, None), ("l3s", 3, 64642, None), ("l3s", 128, 128642, None), ("l3s", 384, 256642, None),
    ("l3d", 2, 64642, None), ("l3d", 3, 64642, None), ("l3d", 128, 128642, None), ("l3d", 129, 128642, None), ("l3d", 384, 256642, None),
    ("l4d", 2, 64642, None), ("l4d", 3, 64642, None), ("l4d", 64, 128642, None), ("l4d", 192, 256642, None), ("l4d", 193, 256642, None),
    ("c96a", 3, 64323, None), ("c96b", 192, 256324, None),
]


@gpu
@pytest.mark.parametrize("layer,n,form,sw", GEMM_CASES, ids=["%s-n%d" % c[:2] for c in GEMM_CASES])
def test_implicit_gemm(eng, defaults, layer, n, form, sw):
    """launch_gemm_f16<A16_IM2COL>: every non-linear build the tile rule picks, at the layers that take it in the forward."""
    check_layer(eng, defaults, layer, n, form, sw)


HALO_OFF_CASES = [("l2", 1, 128323, 642), ("l2", 65, 128323, 1281), ("l3", 2, 64642, 644), ("l3", 3, 64642, 644), ("l3", 130, 128642, 1281),
                  ("l4", 3, 64642, 644), ("l4", 66, 128642, 1281)]


@gpu
@pytest.mark.parametrize("layer,n,form,halo_form", HALO_OFF_CASES, ids=["%s-n%d" % c[:2] for c in HALO_OFF_CASES])
def test_stride1_layers_without_the_halo_kernel(eng, defaults, layer, n, form, halo_form):
    """f16_halo = 0 sends the 3x3 stride-1 layers through the implicit GEMM: within the bound of the oracle, like the halo launch of
    the same operands (the two sum K in different orders: they are not asserted equal)."""
    check_layer(eng, defaults, layer, n, form, {"f16_halo": 0}, seed=700 + n)
    check_layer(eng, defaults, layer, n, halo_form, None, seed=700 + n)


# ----------------------------------------------------------------------------- refusals
REFUSED = [("m % 128", (1, 8, 8, 64), 64), ("cin % 32", (1, 16, 8, 48), 64), ("cout % 64", (1, 16, 8, 64), 96)]


@gpu
@pytest.mark.parametrize("why,xs,cout", REFUSED, ids=[c[0].replace(" ", "") for c in REFUSED])
def test_refused_arguments(eng, defaults, why, xs, cout):
    """What conv_gemm16's launchers refuse comes back as REID_ERR_ARG from their argument checks (no launch); the context stays usable."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(xs, np.float32).astype(np.float16)
    wt = f16(rng.standard_normal((cout, 3, 3, xs[3]), np.float32) / 24)
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.debug_conv_layer_f16(x, wt, 1, 1)
    assert ei.value.status == -1, why
    assert eng.fault_bits() == 0
    check_layer(eng, defaults, "l3", 2, 644)


# ----------------------------------------------------------------------------- layer-1 kernel
def c64_operands(n, seed, dead_image=None):
    """x, folded weights w16 = f16(w32 scale32) [64, 3, 3, 64], residual as float16; shift fp32.  dead_image: x = 0 and a residual so
    negative that conv + shift + residual < 0 everywhere in that image."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 64, 32, 64), np.float32).astype(np.float16)
    x[0, 0, :, :] = 3.0
    x[0, :, 0, :] = -2.0
    w32 = (rng.standard_normal((64, 3, 3, 64), np.float32) / np.float32(24.0)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, 64) * np.where(rng.random(64) < 0.2, -1.0, 1.0)).astype(np.float32)
    w16 = (w32 * scale[:, None, None, None]).astype(np.float16)       # scale_rows_f16_kernel: f16(w * scale), one fp32 product
    shift = rng.normal(0, 0.5, 64).astype(np.float32)
    res = rng.standard_normal((n, 64, 32, 64), np.float32).astype(np.float16)
    if dead_image is not None:
        x[dead_image] = 0
        res[dead_image] = -np.abs(res[dead_image]) - np.float16(4.0)
    return x, w16, shift, res


def c64_images(n):
    return [0] if n == 1 else sorted({0, n - 3, n - 2, n - 1} & set(range(n)))


def c64_oracle(x, w16, imgs):
    rows = np.concatenate([np.arange(i * 2048, (i + 1) * 2048) for i in imgs])
    acc, ab = oracle_rows(x, w16, 1, 1, rows, 2048)
    return rows, acc, ab


def c64_model(acc, ab, shift=None, res=None, relu=False):
    """(v, e) of the fp32 value the kernel sums and rounds: e16 for the raw form, e32 otherwise (module docstring)."""
    ea = SAFETY * 576 * U * ab
    e16 = rounded(acc, ea)
    if shift is None and res is None:
        return acc, e16
    v = epilogue(acc, None, shift, res, relu)
    e = e16 + SAFETY * 4 * U * (np.abs(acc) + (0.0 if shift is None else np.abs(np.asarray(shift, np.float64))) + (0.0 if res is None else np.abs(res)))
    return v, e


C64_CASES = [1, 3, 300]


@gpu
@pytest.mark.parametrize("n", C64_CASES)
def test_c64_kernel(eng, n):
    """launch_conv3x3_c64_f16 without the SE tail, the forward's forms: raw + stats (conv1), folded BN + residual + ReLU with and
    without stats (conv2).  300 images are more than the chip has CUs: the persistent loop."""
    x, w16, shift, res = c64_operands(n, 40 + n)
    imgs = c64_images(n)
    rows, acc, ab = c64_oracle(x, w16, imgs)
    rr = res.reshape(-1, 64)[rows].astype(np.float64)
    pos = {g: list(range(j * 2048, (j + 1) * 2048)) for j, g in enumerate(imgs)}
    out, st, form = eng.debug_conv_c64_se(x, w16.reshape(64, 576), stats=True)
    assert form == 1
    assert np.isfinite(out.astype(np.float32)).all() and np.isfinite(st).all(), "raw: an output was not written"
    v, e = c64_model(acc, ab)
    ratio(out.reshape(-1, 64)[rows], v, e, "c64 n=%d raw" % n)         # the raw form stores the once-rounded accumulator
    vq = out.reshape(-1, 64)[rows].astype(np.float64)                  # ... and sums that f16 value
    group_stats_check(st, imgs, pos, v, e, 2048, "c64 n=%d raw" % n)
    group_stats_check(st, imgs, pos, vq, np.zeros_like(vq), 2048, "c64 n=%d raw, sums of its own output" % n)
    v, e = c64_model(acc, ab, shift, rr, True)
    prev = None
    for stats in (True, False):
        out, st, form = eng.debug_conv_c64_se(x, w16.reshape(64, 576), shift, res, relu=True, stats=stats)
        assert form == 1
        assert np.isfinite(out.astype(np.float32)).all(), "bn+res+relu: an output was not written"
        ratio(out.reshape(-1, 64)[rows], v, rounded(v, e), "c64 n=%d bn+res+relu stats=%d" % (n, stats))
        if stats:
            assert np.isfinite(st).all()
            group_stats_check(st, imgs, pos, v, e, 2048, "c64 n=%d bn+res+relu" % n)
            prev = out
    np.testing.assert_array_equal(out.view(np.uint16), prev.view(np.uint16), err_msg="output with and without stats")


def se_weights(seed):
    """w1 [8, 64] positive (pooled >= 0 after the ReLU, so every hidden unit is alive); w2t [8, 64]: columns 0-15 push the gate towards 1,
    16-31 towards 0, the rest stay in the sigmoid's middle."""
    rng = np.random.default_rng(seed)
    w1 = np.abs(rng.normal(0, 0.05, (8, 64))).astype(np.float32)
    w2t = rng.normal(0, 0.15, (8, 64)).astype(np.float32)
    w2t[:, :16] = np.abs(w2t[:, :16]) * 7
    w2t[:, 16:32] = -np.abs(w2t[:, 16:32]) * 7
    return w1, w2t


SE_CASES = [(2, 1), (3, None), (300, 298)]


@gpu
@pytest.mark.parametrize("n,dead", SE_CASES, ids=["n%d" % c[0] for c in SE_CASES])
def test_c64_fused_se(eng, n, dead):
    """conv2 of a layer-1 block with the SE tail fused (the forward's default, f16_c64 = 2): out = relu(gate y + shortcut), the gate from
    the kernel's own pooled sums.  One image is all negative before the ReLU (pooled = 0, gate = 1/2, output 0)."""
    x, w16, shift, res = c64_operands(n, 60 + n, dead)
    w1, w2t = se_weights(n)
    imgs = c64_images(n)
    rows, acc, ab = c64_oracle(x, w16, imgs)
    rr = res.reshape(-1, 64)[rows].astype(np.float64)
    out, _, form = eng.debug_conv_c64_se(x, w16.reshape(64, 576), shift, res, relu=True, se_w1=w1, se_w2t=w2t)
    assert form == 2
    assert np.isfinite(out.astype(np.float32)).all(), "an output was not written"
    y, e = c64_model(acc, ab, shift, rr, True)
    e_y = rounded(y, e)
    yi, ei = y.reshape(len(imgs), 2048, 64), e.reshape(len(imgs), 2048, 64)
    pooled = yi.sum(1) / 2048
    d_pooled = (ei.sum(1) + SAFETY * 2048 * U * np.abs(yi).sum(1)) / 2048 + U * np.abs(pooled)
    w1d, w2d = w1.astype(np.float64), w2t.astype(np.float64)
    hid = np.maximum(pooled @ w1d.T, 0.0)
    d_h = 64 * U * (np.abs(pooled) @ np.abs(w1d).T) + d_pooled @ np.abs(w1d).T
    g = 1.0 / (1.0 + np.exp(-(hid @ w2d)))
    d_g = SAFETY * (0.25 * (8 * U * (hid @ np.abs(w2d)) + d_h @ np.abs(w2d)) + 4 * U * g)
    alive = [j for j, i in enumerate(imgs) if i != dead]
    assert g[alive, :16].min() > 0.9 and g[alive, 16:32].max() < 0.1, "the SE weights do not saturate the gate"
    gi, dgi = np.repeat(g, 2048, 0), np.repeat(d_g, 2048, 0)
    want = np.maximum(gi * y + rr, 0.0)
    e_o = np.abs(y) * dgi + (gi + dgi) * e_y + SAFETY * 2 * U * (np.abs(gi * y) + np.abs(rr))
    got = out.reshape(-1, 64)[rows]
    ratio(got, want, rounded(want, e_o), "c64 fused SE n=%d" % n)
    short = np.abs(y) * dgi + gi * (H * np.abs(y) + H_ABS) + SAFETY * 2 * U * (np.abs(gi * y) + np.abs(rr))      # the shorter model
    print("c64 fused SE n=%d: max err / shorter model's bound %.3f (not asserted)" % (
        n, (np.abs(got.astype(np.float64) - want) / np.maximum(rounded(want, short), 1e-300)).max()))
    if dead is not None:
        j = imgs.index(dead)
        assert (pooled[j] == 0).all() and (g[j] == 0.5).all()
        assert (out[dead] == 0).all(), "the all-negative image"
