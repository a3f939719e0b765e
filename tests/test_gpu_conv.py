"""The ResNet trunk's convolutions layer by layer, each launch form against a float64 oracle (debug harness reid_debug_conv_layer).

Every launch goes through conv_gemm, as in the forward, with the context's precision and switches; the form a (layer, batch) pair
reaches is proven by bit identity with the same launch under switches that force that form, and by a difference from its
neighbour where the K order differs.  Run on an MI355X: pytest -m gpu tests/test_gpu_conv.py.

Oracle.  A float64 convolution of the fp32 operands, then v = acc * scale + shift (+ res), ReLU on columns >= relu_from; along
with it A = sum |x| |w| per output element (the same convolution on absolute values).  Large launches are checked on a seeded
sample of output rows that always holds whole 128-row groups (the first and the last, so a ragged last 256-row tile), the first
and last row of every 256-row tile, and every edge row and column (the padding) of the first and last image.
test_sampled_oracle_equals_dense_oracle checks the sampled oracle against the dense one bit for bit.

Error bound, per element (derived from the error model, not from observed numbers; u = 2^-24).
  * fp32-class mode (precision 2): x = xh + xl' 2^-11 and w = wh + wl' 2^-11 as f16; the kernels form xh.wh + xh.wl' + xl'.wh and
    drop xl'.wl'.  The dropped product is <= 2^-22 |x||w|, the roundings of xl' and wl' add 2^-22 |x||w| each: 3 * 2^-22 relative
    per product.  Below f16's normal range xl' rounds to an absolute 2^-25 2^-11 = 2^-36 at worst: 2^-36 sum|w| more (x side;
    the weights here stay normal).  Precision 0 multiplies fp32 exactly: no split term.
  * fp32 accumulation over K = R S Cin: at most K u sum|x||w| (split-K partials change the order, not the bound).
  * The epilogue: acc * scale, + shift, + residual: a few u (|acc scale| + |shift| + |res|); we take 4u.  ReLU is 1-Lipschitz.
  * The loader's input affine (exact-fp32 path): relu(x a + b) is off by 2u (|x a| + |b|), which widens A to the convolution of
    (|x a| + |b|) with |w| and adds 2u of it.
  bound = SAFETY * (|scale| ((3 2^-22 + K u) A + 2^-36 sum|w|) + 4u (|acc scale| + |shift| + |res|)), SAFETY = 2 (chosen).
  Column sums of 128 rows (stats): 128 u sum|v| for the sum, 129 u sum v^2 for the sum of squares, times SAFETY.
"""
import numpy as np
import pytest

from reid_amd import _ffi, synth, weights

gpu = pytest.mark.gpu

U = 2.0 ** -24
E_SPLIT = 3 * 2.0 ** -22
ABS_X = 2.0 ** -36
SAFETY = 2.0
N_RANDOM_ROWS = 64          # seeded rows on top of the structural ones (chosen)
ROW_BLOCK = 64              # the oracle's matmul shape: fixed, so a row's float64 result does not depend on the sample

# name: (h, w, cin, cout, r, stride, pad) of the convolutions at 256 x 128 crops (layer 4: stride forced to 1)
LAYERS = {
    "l1": (64, 32, 64, 64, 3, 1, 1),
    "l2": (32, 16, 128, 128, 3, 1, 1), "l2s": (64, 32, 64, 128, 3, 2, 1), "l2d": (64, 32, 64, 128, 1, 2, 0),
    "l3": (16, 8, 256, 256, 3, 1, 1), "l3s": (32, 16, 128, 256, 3, 2, 1), "l3d": (32, 16, 128, 256, 1, 2, 0),
    "l4a": (16, 8, 256, 512, 3, 1, 1), "l4": (16, 8, 512, 512, 3, 1, 1), "l4d": (16, 8, 256, 512, 1, 1, 0),
}
SWITCHES = ("split_x3_small", "x3_unroll", "x3_sk_cap", "x3_narrow", "x3_l4_narrow_nmt", "f16_split_k", "split_x3_min_blocks",
            "conv_x3s", "x3s_sk_cap", "split_gemm_min_tiles", "f32_split_k", "f32_conv", "split_x3")


# ----------------------------------------------------------------------------- float64 oracle
def _padded(x, pad):
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c), np.float64)
    xp[:, pad:pad + h, pad:pad + w] = x
    return xp


def _patches(xp, r, stride, pad, rows):
    n, hp, wp, c = xp.shape
    ho, wo = (hp - r) // stride + 1, (wp - r) // stride + 1
    img, rem = np.divmod(rows, ho * wo)
    oy, ox = np.divmod(rem, wo)
    iy = oy[:, None] * stride + np.arange(r)[None]
    ix = ox[:, None] * stride + np.arange(r)[None]
    return xp[img[:, None, None], iy[:, :, None], ix[:, None, :]].reshape(len(rows), -1)


def conv_oracle(x, w, stride, pad, rows, xabs=None):
    """float64 (acc, A) on the output rows `rows` (flat NHWC row indices): acc = conv(x, w), A = conv(xabs or |x|, |w|).
    x may already hold the loader's affine (float64); padding is zero."""
    cout, r = w.shape[0], w.shape[1]
    wk = w.reshape(cout, -1).astype(np.float64).T
    xa = _padded(np.abs(np.asarray(x, np.float64)) if xabs is None else xabs, pad)
    xp = _padded(x, pad)
    acc = np.empty((len(rows), cout))
    ab = np.empty_like(acc)
    for i in range(0, len(rows), ROW_BLOCK):
        blk = rows[i:i + ROW_BLOCK]
        full = np.concatenate([blk, np.repeat(blk[-1:], ROW_BLOCK - len(blk))])
        acc[i:i + len(blk)] = (_patches(xp, r, stride, pad, full) @ wk)[:len(blk)]
        ab[i:i + len(blk)] = (_patches(xa, r, stride, pad, full) @ np.abs(wk))[:len(blk)]
    return acc, ab


def epilogue(acc, scale=None, shift=None, res=None, relu=False, relu_from=0):
    v = acc * (1.0 if scale is None else np.asarray(scale, np.float64)) + (0.0 if shift is None else np.asarray(shift, np.float64))
    if res is not None:
        v = v + res
    if relu:
        v[:, relu_from:] = np.maximum(v[:, relu_from:], 0.0)
    return v


def bound(acc, ab, w, k, split, scale=None, shift=None, res=None, e_in=0.0):
    sc = np.ones(acc.shape[1]) if scale is None else np.abs(np.asarray(scale, np.float64))
    sh = 0.0 if shift is None else np.abs(np.asarray(shift, np.float64))
    w1 = np.abs(w.astype(np.float64)).reshape(w.shape[0], -1).sum(1)
    mul = (E_SPLIT if split else 0.0) + k * U + e_in
    b = sc * (mul * ab + (ABS_X * w1 if split else 0.0)) + 4 * U * (np.abs(acc * sc) + sh + (0.0 if res is None else np.abs(res)))
    return SAFETY * b


def sample_rows(n, ho, wo, seed, dense_below=4096):
    """Output rows to check: all of them for small launches, else the structural sample of the module docstring."""
    m = n * ho * wo
    if m <= dense_below:
        return np.arange(m)
    rng = np.random.default_rng(seed)
    groups = m // 128
    pick = {0, groups - 1, int(rng.integers(groups))}
    rows = [np.arange(g * 128, g * 128 + 128) for g in pick]
    t0 = np.arange(0, m, 256)
    rows += [t0, np.minimum(t0 + 255, m - 1), np.minimum(t0 + 127, m - 1), np.minimum(t0 + 128, m - 1)]
    oy, ox = np.divmod(np.arange(ho * wo), wo)
    edge = np.nonzero((oy == 0) | (oy == ho - 1) | (ox == 0) | (ox == wo - 1))[0]
    rows += [edge, (n - 1) * ho * wo + edge]
    rows.append(rng.choice(m, N_RANDOM_ROWS, replace=False))
    return np.unique(np.concatenate(rows))


def operands(layer, n, seed, xfn=None):
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32) if xfn is None else xfn(rng, (n, h, w, cin))
    wt = (rng.normal(size=(cout, r, r, cin)) / np.sqrt(r * r * cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(size=cout).astype(np.float32)
    return x, wt, scale, shift, rng


def check_against_oracle(got, x, wt, stride, pad, rows, split, scale=None, shift=None, res=None, relu=False, relu_from=0,
                         xin=None, xabs=None, e_in=0.0, what=""):
    """got [n, ho, wo, cout] (or [m, cout]) against the oracle on `rows`; returns (v_oracle, bound) on those rows."""
    k = wt.shape[1] * wt.shape[2] * wt.shape[3]
    acc, ab = conv_oracle(x if xin is None else xin, wt, stride, pad, rows, xabs)
    rr = None if res is None else res.reshape(-1, wt.shape[0])[rows].astype(np.float64)
    v = epilogue(acc, scale, shift, rr, relu, relu_from)
    b = bound(acc, ab, wt, k, split, scale, shift, rr, e_in)
    g = got.reshape(-1, wt.shape[0])[rows].astype(np.float64)
    err = np.abs(g - v)
    assert np.isfinite(g).all(), "%s: non-finite output" % what
    worst = np.unravel_index(np.argmax(err / b), err.shape)
    assert (err <= b).all(), "%s: row %d col %d: got %r, float64 %r, bound %g" % (
        what, rows[worst[0]], worst[1], g[worst], v[worst], b[worst])
    return v, b


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    sd = synth.seres18_state_dict(0)              # a loaded checkpoint: its zero page lets precision 2 take the split path
    blob, manifest, _ = weights.pack_seres18(sd)
    e.load_seres18(blob, manifest)
    return e


@pytest.fixture(scope="module")
def defaults(eng):
    return {k: eng.debug_switch(k) for k in SWITCHES}


def run(eng, defaults, precision, layer, x, wt, switches=None, **kw):
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    eng.set_precision(precision)
    try:
        for k, v in (switches or {}).items():
            eng.debug_switch(k, v)
        return eng.debug_conv_layer(x, wt, stride, pad, **kw)
    finally:
        for k in (switches or {}):
            eng.debug_switch(k, defaults[k])
        eng.set_precision(0)


def out_shape(layer, n):
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1


# ----------------------------------------------------------------------------- CPU: the sampled oracle
def test_sampled_oracle_equals_dense_oracle():
    """The row-restricted oracle is the dense one, bit for bit, on a sample with every structural part (ragged tail included)."""
    for layer, n in (("l4", 5), ("l2s", 3)):
        x, wt, _, _, _ = operands(layer, n, 11)
        h, w, cin, cout, r, stride, pad = LAYERS[layer]
        ho, wo = out_shape(layer, n)
        dense, dab = conv_oracle(x, wt, stride, pad, np.arange(n * ho * wo))
        rows = sample_rows(n, ho, wo, 3, dense_below=0)
        assert len(rows) < n * ho * wo and rows[-1] == n * ho * wo - 1 and 0 in rows
        acc, ab = conv_oracle(x, wt, stride, pad, rows)
        np.testing.assert_array_equal(acc, dense[rows])
        np.testing.assert_array_equal(ab, dab[rows])
        # and the oracle is a convolution: torch's float64 conv2d on a few rows
        import torch
        ref = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2),
                                         torch.from_numpy(wt.astype(np.float64)).permute(0, 3, 1, 2), None, stride, pad)
        ref = ref.permute(0, 2, 3, 1).reshape(-1, cout).numpy()
        np.testing.assert_allclose(dense, ref, rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------- launch forms
# (layer, batch, form, switch sets that must give the same bits, switch sets that must not).  The batch sizes sit on both sides of
# the selection rules: conv3x3_x3_supported (layer 1 from 33 crops, layer 2 from 65), x3_wide_tiles (layer 3: 64-wide below 63
# crops; layer 4: 64-wide at 33..62, 65..96 and 129..192), x3_split (1/2/4 ways; 8 only under x3_sk_cap), launch_conv_x3s's
# split, conv_split_path (strided 3x3 from 96 / 48 tile rows of 128 columns, 1x1 from 128), launch_bn's split in conv_f32.hip.
NAR = {"x3_narrow": 3}
WIDE4 = {"x3_l4_narrow_nmt": 0}
FORMS = [
    ("l1", 2, "12-wave, split K", [{"split_x3_small": 0}], [{"split_x3_small": 1}, {"f16_split_k": 0}]),
    ("l1", 32, "12-wave", [{"split_x3_small": 0}, {"f16_split_k": 0}], [{"split_x3_small": 1}]),
    ("l1", 33, "x3u 64-wide", [{"split_x3_small": 1}, {"x3_unroll": 0}], [{"split_x3_small": 0}]),
    ("l2", 8, "12-wave, split K", [{"split_x3_small": 0}], [{"split_x3_small": 1}, {"f16_split_k": 0}]),
    ("l2", 64, "12-wave", [{"split_x3_small": 0}, {"f16_split_k": 0}], [{"split_x3_small": 1}]),
    ("l2", 65, "x3u 64-wide", [{"split_x3_small": 1}, {"x3_unroll": 0}], [{"split_x3_small": 0}]),
    ("l2", 66, "x3u 64-wide", [{"split_x3_small": 1}, {"x3_unroll": 0}], [{"split_x3_small": 0}]),
    ("l3", 3, "x3 64-wide, 4-way", [NAR, {"x3_sk_cap": 4}, {"x3_unroll": 0}], [{"x3_sk_cap": 2}, {"x3_sk_cap": 1}]),
    ("l3", 61, "x3 64-wide, 4-way", [NAR, {"x3_sk_cap": 4}, {"x3_unroll": 0}], [{"x3_sk_cap": 2}, {"x3_sk_cap": 8}]),
    ("l3", 63, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, {"x3_unroll": 0}, {"x3_narrow": 5}], [{"x3_sk_cap": 2}]),
    ("l3", 65, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, {"x3_narrow": 5}], [NAR, {"x3_sk_cap": 2}]),
    ("l3", 129, "x3 128-wide, 2-way", [{"x3_sk_cap": 2}, {"x3_unroll": 0}], [{"x3_sk_cap": 1}, NAR]),
    ("l4", 3, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, {"x3_unroll": 0}], [{"x3_sk_cap": 2}, {"x3_sk_cap": 8}]),
    ("l4", 32, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, {"x3_unroll": 0}, WIDE4], [{"x3_sk_cap": 2}, {"x3_sk_cap": 8}]),
    ("l4", 33, "x3 64-wide, 2-way", [NAR, {"x3_sk_cap": 2}, {"x3_unroll": 0}], [WIDE4, {"x3_sk_cap": 1}]),
    ("l4", 62, "x3 64-wide, 2-way", [NAR, {"x3_sk_cap": 2}], [WIDE4]),
    ("l4", 63, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, WIDE4], [NAR, {"x3_sk_cap": 2}]),
    ("l4", 64, "x3 128-wide, 4-way", [{"x3_sk_cap": 4}, WIDE4, {"x3_unroll": 0}], [NAR, {"x3_sk_cap": 2}]),
    ("l4", 65, "x3 64-wide, 2-way (= 128-wide)", [NAR, WIDE4, {"x3_sk_cap": 2}], [{"x3_sk_cap": 1}]),
    ("l4", 96, "x3 64-wide, 2-way (= 128-wide)", [NAR, WIDE4, {"x3_sk_cap": 2}], [{"x3_sk_cap": 1}]),
    ("l4", 97, "x3 128-wide, 2-way", [WIDE4, {"x3_sk_cap": 2}], [NAR, {"x3_sk_cap": 1}]),
    ("l4", 128, "x3 128-wide, 2-way", [WIDE4, {"x3_sk_cap": 2}, {"x3_unroll": 0}], [NAR]),
    ("l4", 129, "x3 64-wide, unsplit (= 128-wide)", [NAR, WIDE4, {"x3_sk_cap": 1}], [{"split_x3_small": 0}]),
    ("l4", 192, "x3 64-wide, unsplit (= 128-wide)", [NAR, WIDE4, {"x3_sk_cap": 1}], [{"split_x3_small": 0}]),
    ("l4", 193, "x3 128-wide, unsplit", [WIDE4, {"x3_sk_cap": 1}, {"x3_unroll": 0}], [{"split_x3_small": 0}]),
    ("l4a", 33, "x3 64-wide, 2-way", [NAR, {"x3_sk_cap": 2}], [WIDE4]),
    ("l4a", 65, "x3 64-wide, 2-way (= 128-wide)", [NAR, WIDE4], [{"x3_sk_cap": 1}]),
    ("l2s", 47, "exact fp32 conv_f32, split K", [{"split_gemm_min_tiles": 1000000}, {"conv_x3s": 0}], [{"f32_split_k": 0}, {"conv_x3s": 2}]),
    ("l2s", 48, "conv_x3s, 4-way", [{"x3s_sk_cap": 4}, {"split_gemm_min_tiles": 1}], [{"x3s_sk_cap": 2}, {"conv_x3s": 0},
                                                                                      {"split_gemm_min_tiles": 1000000}]),
    ("l2d", 63, "exact fp32 conv_f32", [{"split_gemm_min_tiles": 1000000}, {"f32_split_k": 0}], [{"conv_x3s": 2}]),
    ("l2d", 64, "conv_x3s, unsplit", [{"x3s_sk_cap": 1}, {"f16_split_k": 0}], [{"conv_x3s": 0}, {"split_gemm_min_tiles": 1000000}]),
    ("l3s", 16, "exact fp32 conv_f32, split K", [{"split_gemm_min_tiles": 1000000}], [{"f32_split_k": 0}, {"split_gemm_min_tiles": 1}]),
    ("l3s", 95, "exact fp32 conv_f32, split K", [{"split_gemm_min_tiles": 1000000}], [{"f32_split_k": 0}, {"conv_x3s": 2}]),
    ("l3s", 96, "conv_x3s, 4-way", [{"x3s_sk_cap": 4}, {"split_gemm_min_tiles": 1}], [{"x3s_sk_cap": 2}, {"conv_x3s": 0}]),
    ("l3d", 127, "exact fp32 conv_f32", [{"split_gemm_min_tiles": 1000000}, {"f32_split_k": 0}], [{"conv_x3s": 2}]),
    ("l3d", 129, "conv_x3s, 2-way", [{"x3s_sk_cap": 2}], [{"x3s_sk_cap": 1}, {"conv_x3s": 0}]),
    ("l4d", 63, "exact fp32 conv_f32", [{"split_gemm_min_tiles": 1000000}], [{"conv_x3s": 2}]),
    ("l4d", 64, "conv_x3s, 4-way", [{"x3s_sk_cap": 4}], [{"x3s_sk_cap": 2}, {"conv_x3s": 0}]),
    ("l4d", 65, "conv_x3s, 2-way", [{"x3s_sk_cap": 2}], [{"x3s_sk_cap": 1}, {"conv_x3s": 0}]),
    ("l4d", 129, "conv_x3s, unsplit", [{"x3s_sk_cap": 1}], [{"conv_x3s": 0}]),
]


@gpu
@pytest.mark.parametrize("layer,n,form,same,differ", FORMS, ids=["%s-n%d" % (f[0], f[1]) for f in FORMS])
def test_launch_form(eng, defaults, layer, n, form, same, differ):
    """The default launch equals the forced form bit for bit, differs from its neighbour, and is within the bound of the oracle
    (BN + ReLU epilogue).  Forms that take the exact-fp32 kernel are held to the precision-0 bound."""
    x, wt, sc, sh, _ = operands(layer, n, 1000 + n)
    kw = dict(scale=sc, shift=sh, relu=True)
    got = run(eng, defaults, 2, layer, x, wt, **kw)[0]
    for sw in same:
        np.testing.assert_array_equal(run(eng, defaults, 2, layer, x, wt, sw, **kw)[0], got, err_msg="%s: %s" % (form, sw))
    for sw in differ:
        assert not np.array_equal(run(eng, defaults, 2, layer, x, wt, sw, **kw)[0], got), "%s: same bits under %s" % (form, sw)
    ho, wo = out_shape(layer, n)
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    check_against_oracle(got, x, wt, stride, pad, sample_rows(n, ho, wo, n), "exact fp32" not in form, sc, sh, relu=True,
                         what="%s n=%d (%s)" % (layer, n, form))


# ----------------------------------------------------------------------------- epilogues
# one launch per form of the epilogue code: the 12-wave kernel, x3m16_tail unsplit / split, conv_x3s, exact fp32 (ragged tails: odd n
# at 16 x 8 maps)
EPI_CASES = [("l1", 2, 2), ("l1", 33, 2), ("l2", 65, 2), ("l3", 3, 2), ("l4", 33, 2), ("l4", 129, 2), ("l4", 3, 2), ("l2s", 48, 2),
             ("l4d", 65, 2), ("l3s", 3, 2), ("l3", 3, 0), ("l4", 33, 0)]


@gpu
@pytest.mark.parametrize("layer,n,prec", EPI_CASES, ids=["%s-n%d-p%d" % c for c in EPI_CASES])
def test_epilogue_variants(eng, defaults, layer, n, prec):
    """Raw output, BN, BN + ReLU, BN + residual + ReLU against the oracle; the raw launch's stats against float64 sums."""
    x, wt, sc, sh, rng = operands(layer, n, 2000 + n)
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    ho, wo = out_shape(layer, n)
    res = rng.normal(size=(n, ho, wo, cout)).astype(np.float32)
    rows = sample_rows(n, ho, wo, n + 7)
    split = prec == 2 and not (layer.endswith(("s", "d")) and n < 48)
    for name, kw in (("raw", {}), ("bn", dict(scale=sc, shift=sh)), ("bn+relu", dict(scale=sc, shift=sh, relu=True)),
                     ("bn+res+relu", dict(scale=sc, shift=sh, residual=res, relu=True))):
        got = run(eng, defaults, prec, layer, x, wt, **kw)[0]
        check_against_oracle(got, x, wt, stride, pad, rows, split, kw.get("scale"), kw.get("shift"), kw.get("residual"),
                             kw.get("relu", False), what="%s n=%d %s" % (layer, n, name))


def check_stats(stats, v32, what):
    """stats [m/128, cout, 2] against float64 sums of the kernel's own fp32 v over each 128-row group (all groups written)."""
    assert np.isfinite(stats).all(), "%s: a stats group was not written" % what
    g = v32.reshape(-1, 128, v32.shape[-1]).astype(np.float64)
    s1, s2 = g.sum(1), (g * g).sum(1)
    b1, b2 = SAFETY * 128 * U * np.abs(g).sum(1), SAFETY * 129 * U * (g * g).sum(1)
    assert (np.abs(stats[..., 0] - s1) <= b1 + 1e-30).all(), "%s: column sums" % what
    assert (np.abs(stats[..., 1] - s2) <= b2 + 1e-30).all(), "%s: column sums of squares" % what


def check_packed(pk, v32, pack_from, what):
    """[yh | yl'] bit for bit: yh = f16(v), yl' = f16((v - yh) 2^11) of the kernel's own fp32 v, columns >= pack_from only."""
    c = v32.shape[-1]
    v = v32.reshape(-1, c)[:, pack_from:]
    yh = v.astype(np.float16)
    yl = ((v - yh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    np.testing.assert_array_equal(pk[:, pack_from:c], yh.view(np.uint16), err_msg="%s: yh" % what)
    np.testing.assert_array_equal(pk[:, c + pack_from:], yl.view(np.uint16), err_msg="%s: yl'" % what)
    assert (pk[:, :pack_from] == 0xffff).all() and (pk[:, c:c + pack_from] == 0xffff).all(), "%s: packed store below pack_from" % what


IBN_CASES = [("l1", 2), ("l1", 33), ("l2", 8), ("l2", 65), ("l3", 3), ("l3", 61), ("l4", 3), ("l4", 33), ("l4", 129), ("l4d", 65)]


@gpu
@pytest.mark.parametrize("layer,n", IBN_CASES, ids=["%s-n%d" % c for c in IBN_CASES])
def test_ibn_packed_and_stats(eng, defaults, layer, n):
    """IBN conv1: ReLU and the [yh | yl'] store from C/2 on, stats on; and packed output from column 0 (layer 4's conv1).  The packed
    form matches the kernel's own fp32 v bit for bit, yh + yl' 2^-11 the oracle; stats the float64 sums of v and of the oracle."""
    x, wt, sc, sh, _ = operands(layer, n, 3000 + n)
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    ho, wo = out_shape(layer, n)
    half = cout // 2
    what = "%s n=%d" % (layer, n)
    for pack_from in (half, 0):
        kw = dict(scale=sc, shift=sh, relu=True, relu_from=pack_from, stats=True)
        v32, none, st_plain = run(eng, defaults, 2, layer, x, wt, **kw)
        assert none is None
        out, pk, st = run(eng, defaults, 2, layer, x, wt, pack_from=pack_from, **kw)
        assert pk is not None, "%s: the packed store was not made" % what
        np.testing.assert_array_equal(out[..., :pack_from], v32[..., :pack_from], err_msg=what)
        assert np.isnan(out[..., pack_from:]).all(), "%s: fp32 store of packed columns" % what
        check_packed(pk, v32, pack_from, what)
        np.testing.assert_array_equal(st, st_plain, err_msg="%s: stats with and without the packed store" % what)
        check_stats(st, v32, what)
        # against the oracle: v everywhere, yh + yl' 2^-11 on the packed columns, and the stats of whole sampled groups
        groups = np.array(sorted({0, n * ho * wo // 128 - 1, (n * ho * wo // 128) // 2}))
        rows = np.unique(np.concatenate([sample_rows(n, ho, wo, n)] + [np.arange(g * 128, g * 128 + 128) for g in groups]))
        vo, b = check_against_oracle(v32, x, wt, stride, pad, rows, True, sc, sh, relu=True, relu_from=pack_from, what=what)
        recon = pk[rows, pack_from:cout].view(np.float16).astype(np.float64) + pk[rows, cout + pack_from:].view(np.float16) / 2048.0
        assert (np.abs(recon - vo[:, pack_from:]) <= b[:, pack_from:] + 2.0 ** -21 * np.abs(vo[:, pack_from:]) + 2.0 ** -35).all()
        pos = {g: i for i, g in enumerate(rows)}
        for g in groups:
            idx = [pos[q] for q in range(g * 128, g * 128 + 128)]
            vg, bg = vo[idx], b[idx]
            assert (np.abs(st[g, :, 0] - vg.sum(0)) <= bg.sum(0) + SAFETY * 128 * U * np.abs(vg).sum(0)).all(), what
            assert (np.abs(st[g, :, 1] - (vg * vg).sum(0)) <= (bg * (2 * np.abs(vg) + bg)).sum(0) + SAFETY * 129 * U * (vg * vg).sum(0)).all(), what


# ----------------------------------------------------------------------------- inputs
def wide_rows(rng, shape):
    x = rng.normal(size=shape)
    return (x * 10.0 ** rng.uniform(-6, 3, size=shape[:3] + (1,))).astype(np.float32)


def f16_subnormal(rng, shape):     # |x| in f16's subnormal range (2^-24 .. 2^-14): xh keeps few bits, xl' carries the rest
    return (rng.choice([-1.0, 1.0], size=shape) * 2.0 ** rng.uniform(-24, -14, size=shape)).astype(np.float32)


def zeros_signed(rng, shape):
    x = rng.normal(size=shape).astype(np.float32)
    x[rng.random(shape) < 0.5] = 0.0
    neg = rng.random(shape) < 0.5
    x[(x == 0) & neg] = -0.0
    x[:, :3] = -0.0                  # whole image rows of -0: output row 1 of a 3x3 stride-1 convolution reads nothing else
    return x


INPUT_CASES = [(f, layer, n) for f in ("wide_rows", "f16_subnormal", "zeros_signed") for layer, n in (("l1", 33), ("l3", 3), ("l4", 33), ("l2s", 48), ("l2", 8))]


@gpu
@pytest.mark.parametrize("kind,layer,n", INPUT_CASES, ids=["%s-%s-n%d" % c for c in INPUT_CASES])
def test_inputs(eng, defaults, kind, layer, n):
    x, wt, sc, sh, _ = operands(layer, n, 4000 + n, globals()[kind])
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    ho, wo = out_shape(layer, n)
    got = run(eng, defaults, 2, layer, x, wt)[0]
    check_against_oracle(got, x, wt, stride, pad, sample_rows(n, ho, wo, n), True, what="%s %s n=%d" % (kind, layer, n))
    if kind == "zeros_signed":       # rows whose every tap reads zeros: exactly zero
        zero_in = ~np.any(x != 0, axis=(2, 3))
        if r == 3 and stride == 1:
            dead = zero_in[:, :-2] & zero_in[:, 1:-1] & zero_in[:, 2:]
            assert (got[:, 1:-1][dead] == 0).all()
            assert dead.any()


@gpu
def test_activation_beyond_f16_is_reported_and_cleared(eng, defaults):
    """An activation >= 65504 on the split path raises fault bit 1: the call that made it fails, clear_fault resets it."""
    x, wt, _, _, _ = operands("l4", 3, 5000)
    x[1, 3, 4, 7] = 70000.0
    with pytest.raises(_ffi.ReidHipError) as ei:
        run(eng, defaults, 2, "l4", x, wt)
    assert ei.value.status == -3
    assert eng.fault_bits() & 1
    eng.clear_fault()
    assert eng.fault_bits() == 0
    x[1, 3, 4, 7] = 1.0
    got = run(eng, defaults, 2, "l4", x, wt)[0]
    check_against_oracle(got, x, wt, 1, 1, sample_rows(3, 16, 8, 3), True, what="after clear_fault")


# ----------------------------------------------------------------------------- exact fp32 path
F32_CASES = [("l4", 3, {}), ("l4", 3, {"f32_split_k": 0}), ("l4", 3, {"f32_conv": 0}), ("l1", 2, {}), ("l1", 2, {"f32_split_k": 0}),
             ("l3s", 16, {}), ("l3s", 16, {"f32_split_k": 0}), ("l3s", 16, {"f32_conv": 0}), ("l2d", 5, {}), ("l2d", 5, {"f32_conv": 0})]


@gpu
@pytest.mark.parametrize("layer,n,sw", F32_CASES, ids=["%s-n%d-%s" % (c[0], c[1], "-".join("%s%d" % kv for kv in c[2].items()) or "dflt") for c in F32_CASES])
def test_exact_fp32(eng, defaults, layer, n, sw):
    """Precision 0: conv_f32.hip with and without split K, gemm_f32 A_IM2COL (f32_conv 0); with stats and IBN ReLU."""
    x, wt, sc, sh, rng = operands(layer, n, 6000 + n)
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    ho, wo = out_shape(layer, n)
    kw = dict(scale=sc, shift=sh, relu=True, relu_from=cout // 2, stats=True)
    got, _, st = run(eng, defaults, 0, layer, x, wt, sw, **kw)
    check_against_oracle(got, x, wt, stride, pad, sample_rows(n, ho, wo, n), False, sc, sh, relu=True, relu_from=cout // 2,
                         what="%s n=%d %s" % (layer, n, sw))
    check_stats(st, got, "%s n=%d %s" % (layer, n, sw))


@gpu
@pytest.mark.parametrize("layer,n", [("l4", 3), ("l2", 2), ("l1", 2)])
def test_exact_fp32_input_affine(eng, defaults, layer, n):
    """The loader's per-(image, channel) affine + ReLU that conv2 uses at precision 0 without conv_f32 (gemm_f32 A_IM2COL)."""
    x, wt, sc, sh, rng = operands(layer, n, 7000 + n)
    h, w, cin, cout, r, stride, pad = LAYERS[layer]
    ho, wo = out_shape(layer, n)
    asc = rng.uniform(-2, 2, (n, cin)).astype(np.float32)
    ash = rng.normal(size=(n, cin)).astype(np.float32)
    xin = np.maximum(x.astype(np.float64) * asc[:, None, None, :] + ash[:, None, None, :], 0.0)
    xabs = np.abs(x.astype(np.float64) * asc[:, None, None, :]) + np.abs(ash[:, None, None, :])
    for sw in ({}, {"f32_conv": 0}):
        got = run(eng, defaults, 0, layer, x, wt, sw, scale=sc, shift=sh, relu=True, a_scale=asc, a_shift=ash, a_relu=True)[0]
        check_against_oracle(got, x, wt, stride, pad, sample_rows(n, ho, wo, n), False, sc, sh, relu=True, xin=xin, xabs=xabs,
                             e_in=2 * U, what="%s n=%d affine %s" % (layer, n, sw))


# ----------------------------------------------------------------------------- determinism
DET_CASES = [("l1", 2, 2, {}), ("l4", 3, 2, {}), ("l4", 33, 2, {}), ("l4", 3, 2, {"x3_sk_cap": 8}), ("l2s", 48, 2, {}),
             ("l4d", 65, 2, {}), ("l3s", 16, 2, {"split_gemm_min_tiles": 1}), ("l3s", 16, 0, {}), ("l4", 3, 0, {})]


@gpu
@pytest.mark.parametrize("layer,n,prec,sw", DET_CASES, ids=["%s-n%d-p%d-%d" % (c[0], c[1], c[2], i) for i, c in enumerate(DET_CASES)])
def test_split_k_is_deterministic(eng, defaults, layer, n, prec, sw):
    """Three repeats of each split-K launch (x3 2/4/8 ways, conv_x3s, the 12-wave kernel, conv_f32) are bit-identical, stats included."""
    x, wt, sc, sh, _ = operands(layer, n, 8000 + n)
    outs = [run(eng, defaults, prec, layer, x, wt, sw, scale=sc, shift=sh, relu=True, stats=True) for _ in range(3)]
    for o, _, s in outs[1:]:
        np.testing.assert_array_equal(o, outs[0][0])
        np.testing.assert_array_equal(s, outs[0][2])
    if sw:
        h, w, cin, cout, r, stride, pad = LAYERS[layer]
        ho, wo = out_shape(layer, n)
        check_against_oracle(outs[0][0], x, wt, stride, pad, sample_rows(n, ho, wo, n), prec == 2, sc, sh, relu=True,
                             what="%s n=%d %s" % (layer, n, sw))


# ----------------------------------------------------------------------------- reid_conv2d_nhwc
@gpu
def test_conv2d_nhwc_split_weights_follow_the_call(eng, defaults):
    """Precision 2: two calls with different weights of one shape, each against float64 (the split form cached under the reused
    weight workspace belonged to the first call)."""
    eng.set_precision(2)
    try:
        for seed in (1, 2, 3):
            x, wt, sc, sh, _ = operands("l4", 3, 9000 + seed)
            got = eng.conv2d_nhwc(x, wt, 1, 1, sc, sh)
            check_against_oracle(got, x, wt, 1, 1, sample_rows(3, 16, 8, seed), True, sc, sh, what="call %d" % seed)
    finally:
        eng.set_precision(0)


@gpu
def test_conv2d_nhwc_refuses_unsplittable_weights(eng, defaults):
    x, wt, _, _, _ = operands("l4", 3, 9100)
    wt[5, 1, 1, 3] = 40.0               # 40 * 2^11 > 65504
    eng.set_precision(2)
    try:
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.conv2d_nhwc(x, wt, 1, 1)
        assert ei.value.status == -1 and "65504" in str(ei.value)
        assert eng.fault_bits() == 0
    finally:
        eng.set_precision(0)
    got = eng.conv2d_nhwc(x, wt, 1, 1)      # mode 0 takes them
    check_against_oracle(got, x, wt, 1, 1, sample_rows(3, 16, 8, 1), False, what="mode 0")


@gpu
def test_conv2d_nhwc_reports_its_fault(eng, defaults):
    x, wt, _, _, _ = operands("l4", 3, 9200)
    x[0, 0, 0, 0] = -1e5
    eng.set_precision(2)
    try:
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.conv2d_nhwc(x, wt, 1, 1)
        assert ei.value.status == -3
    finally:
        eng.clear_fault()
        eng.set_precision(0)
    assert eng.fault_bits() == 0
