"""The front end of a ResNet pass kernel by kernel against float64: resize, every stem form, max-pool (debug harnesses reid_debug_stem,
reid_debug_resize_norm, reid_debug_maxpool).  Every launch goes through the launcher the forward calls.  Run on an MI355X:
pytest -m gpu tests/test_gpu_frontend.py (-s prints the worst err / bound of every case, "RATIO <family> ...").

Oracle.  x = (2v - 255) / 255 for a uint8 crop (the fp32 entry gets float32(x) and is measured against that), acc = the 7x7 stride-2
pad-3 convolution with zero padding in NORMALISED units, v = acc * scale + shift, then MaxPool(3, 2, 1) with -inf padding, all float64.
Beside it A = conv(|x|, |w|), X1 = conv(|x|, 1) and, per output position, W1 = the sum of |w| over the taps inside the image.
test_oracle_is_torch_conv_and_pool pins it to torch's float64 conv2d + max_pool2d.  Batches of more than 8 crops are checked on
images 0 .. 3 (the fixed crops below), n - 1 and two seeded ones (test_sampled_images_equal_dense); every other image must be
finite, i.e. written (the harness fills outputs with NaN).

Inputs.  Image 0 is one fixed crop in every batch: noise with an all-0 band and an all-255 band that touch three borders, and a zero
frame inside a non-zero last row and last column.  From 4 crops on, images 1 .. 3 are an all-0 crop, an all-255 crop (the padding
is 0 in normalised units, i.e. neither) and a crop whose only non-zero pixels are its last row and column (the uint8 loader's
clamped second dword).  shift is -8 on half the channels and +8 on the rest, scale has a random sign: whole maps are negative, so a
pool that pads with 0 instead of -inf is off by about 8 at every border and seam it touches
(test_zero_padded_or_seamed_pool_would_fail shows that on the CPU for every bound below).

Strips.  launch_stem_split and launch_stem_f32 keep the strip / tile count they choose to themselves and the harness does not touch
them, so split_strips() and f32_tiles_per_block() RESTATE the two rules; test_strip_rules pins the table the cases rely on.  That the
launch really takes that many strips is not observable from outside; what is checked is that every batch size that the rule sends
to a different strip count gives the oracle's values and, for image 0, the same bits.

Error bounds, per element, derived from the arithmetic and not from observed numbers.  u = 2^-24, K = 147, h = 2^-11 (f16 half
ulp), f16 below its normal range rounds to an absolute 2^-25.  s = |scale|.  SAFETY = 2 (the factor tests/test_gpu_conv.py chose)
multiplies every bound.  A POOLED element's bound is the maximum of the bounds in its 3x3 window: max is 1-Lipschitz in the sup norm.
  * epilogue, all modes: acc * scale, + shift, and in stem_split the sum of the accumulators and scale / 255: at most four fp32
    roundings of |acc s| and one of |v|: 4u (|acc s| + |shift|).
  * uint8 loaders of the fp32 and f16 paths compute (float(v) / 255 - 0.5) / 0.5: one rounding of v / 255 <= 1 and one of the
    difference, the division by 0.5 is exact: |x' - x| <= 2u, so e_in = 2u s W1.  fp32 input: e_in = 0.
  * mode 0 (stem_f32_kernel, forms 0 / 1; generic A_STEM_* GEMM, form 6): exact fp32 products, K fp32 accumulations:
        b0 = s K u A + e_in + epilogue.
  * mode 2, fp32 input (stem_split_kernel<false>): x = xh + xl' 2^-11, w = wh + wl' 2^-11; the kernel forms xh wh + (xl' wh + xh wl')
    2^-11 and drops xl' wl' 2^-22.  Dropped product <= 2^-22 |x||w|, the f16 roundings of xl' and wl' 2^-22 |x||w| each: 3 2^-22.
    xl' or wl' below f16's normal range rounds to 2^-25 2^-11 = 2^-36 absolute: 2^-36 (W1 + X1).  Main accumulator K roundings, the
    correction accumulator 2K roundings of terms <= 2 |x||w| scaled by 2^-11: K u (1 + 2^-9).
        b2f = s ((3 2^-22 + K u (1 + 2^-9)) A + 2^-36 (W1 + X1)) + epilogue.
  * mode 2, uint8 input (stem_split_kernel<true>): the operand is the INTEGER 2v - 255, exact in f16, so no x split and no dropped
    product; the weight is wh + wl' 2^-11 + wll' 2^-22 with the residuals formed exactly in fp32, so what remains is the f16 rounding
    of wll': 2^-11 2^-22 = 2^-33 |w| relative, 2^-25 2^-22 = 2^-47 absolute below f16's normal range; three accumulators, the two
    corrections scaled by 2^-11 and 2^-22: K u (1 + 2^-10).  1 / 255 is folded into the scale (one rounding, in the epilogue's four).
        b2u = s ((2^-33 + K u (1 + 2^-10)) A + 2^-47 X1) + epilogue.
  * packed output [xh | xl']: bit for bit the split of the kernel's own fp32 value; xh + xl' 2^-11 is within 2^-22 |v| + 2^-36 of it.
  * mode 1, fused kernel (stem_pool_f16_kernel, forms 3 / 4): weights f16(fl32(w scale)): h + u; x f16: h (uint8: after e_in); fp32
    accumulation K u; weights below f16's normal range 2^-25 X1.  The kernel then stores the conv tile as f16 BEFORE the shift:
    h |acc s| + 2^-25, pools, and stores f16(fl32(max + shift)): (h + u) |v| + 2^-25.
        b1 = s (2h + h^2 + 2u + K u) A + e_in + 2^-25 X1 + h |acc s| + (h + u) |v| + 2 2^-25.
  * mode 1, unfused (prep + gemm_f16 A16_STEM + maxpool3s2_f16, form 5): weights f16(w): h, x: h, fp32 accumulation, fp32
    acc * scale + shift (the epilogue term), one f16 store:
        b5 = s ((2h + h^2 + K u) A + 2^-25 X1) + e_in + epilogue + h |v| + 2^-25.
  * max-pool kernels alone: exact.
  * form 1 against reid_debug_maxpool of form 0: bit equality is asserted.  Both builds of stem_f32_kernel issue the same MFMAs in
    the same order on the same LDS image and evaluate the same expression acc * scale + shift; a strip's tile count does not enter a
    tile's arithmetic.  Forms 3 and 4 (uint8 input) run the same kernel on the same f16 values: bit equality.  Form 6 at precisions 0
    and 2: conv_gemm sends A_STEM_* to the exact-fp32 GEMM in both: bit equality.
  * resize_norm_kernel: bit equality with oracle.matching.preprocess (numpy fp32, the same unfused operations in the same order).
    Against the float64 restatement (half-pixel centres, edge clamp, horizontal then vertical): the kernel rounds the tap coordinate
    c to fp32, |c' - c| <= u |c| <= u src (the fraction c' - floor(c') is then exact); the interpolant is continuous and piecewise
    linear with slope at most Dx (Dy): the largest difference of horizontally (vertically) adjacent pixels / 255 among the taps'
    neighbours (rows sy - 1 .. sy + 2, columns sx - 1 .. sx + 2).  The chain: / 255 (u), 1 - f (u), two products and a sum per lerp
    (3u each, values <= 1), - 0.5 (u): 10u at most; / 0.5 doubles everything.
        br = 2 (u (|cx| + 1) Dx + u (|cy| + 1) Dy + 10u).
"""
import numpy as np
import pytest

from reid_amd import _ffi, synth, weights

gpu = pytest.mark.gpu

U = 2.0 ** -24
K = 147
H16 = 2.0 ** -11
H16_ABS = 2.0 ** -25
SAFETY = 2.0
IMG_H, IMG_W, MAP_H, MAP_W, C = 256, 128, 128, 64, 64

# batch sizes -> strips launch_stem_split's rule chooses (every count it can choose), and those with a ragged last strip
SPLIT_N = (1, 5, 9, 12, 17, 20, 24, 26, 33, 37, 43, 52, 74, 103, 214)
SPLIT_STRIPS = (64, 32, 22, 16, 13, 11, 10, 8, 7, 6, 5, 4, 3, 2, 1)
F32_N = (1, 16, 32, 64, 128)


# ----------------------------------------------------------------------------- the launchers' rules, restated
def split_strips(n):
    """launch_stem_split: the strip count of least cost rounds * (3 + 5 * (strip length + 1 redone tile)), first minimum."""
    if n >= 256:
        return 1
    best, nseg = None, 1
    for s in range(1, 65):
        rounds = (n * s + 255) // 256
        cost = rounds * (3 + 5 * ((64 + s - 1) // s + (1 if s > 1 else 0)))
        if best is None or cost < best:
            best, nseg = cost, s
    return nseg


def split_seams(s):
    """First tile (= pooled row) of every strip but the first: strip g covers tiles [g 64 / s, (g + 1) 64 / s)."""
    return sorted({g * 64 // s for g in range(1, s)})


def f32_tiles_per_block(n, pooled):
    t = 64
    while t > (8 if pooled else 1) and n * (64 // t) < 512:
        t >>= 1
    return t


def test_strip_rules():
    assert tuple(split_strips(n) for n in SPLIT_N) == SPLIT_STRIPS
    assert {split_strips(n) for n in range(1, 600)} == set(SPLIT_STRIPS)            # no batch size reaches another count
    assert sorted(s for s in SPLIT_STRIPS if 64 % s) == [3, 5, 6, 7, 10, 11, 13, 22]      # the ragged ones
    assert [f32_tiles_per_block(n, False) for n in F32_N] == [1, 2, 4, 8, 16]
    assert [f32_tiles_per_block(n, True) for n in F32_N] == [8, 8, 8, 8, 16]
    assert split_seams(3) == [21, 42] and split_seams(1) == []


# ----------------------------------------------------------------------------- operands
def stem_operands():
    rng = np.random.default_rng(20240)
    w = (rng.normal(size=(C, 7, 7, 3)) / np.sqrt(K)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = np.full(C, 8.0, np.float32)
    shift[rng.permutation(C)[:C // 2]] = -8.0
    return w, scale, shift


W, SCALE, SHIFT = stem_operands()


def fixed_crops():
    rng = np.random.default_rng(7)
    c0 = rng.integers(0, 256, (IMG_H, IMG_W, 3), dtype=np.uint8)
    c0[0:16] = 0
    c0[16:32] = 255
    c0[248:255, :] = 0
    c0[:, 120:127] = 0
    c0[255] |= 1
    c0[:, 127] |= 1
    last = np.zeros_like(c0)
    last[255] = rng.integers(1, 256, (IMG_W, 3), dtype=np.uint8)
    last[:, 127] = rng.integers(1, 256, (IMG_H, 3), dtype=np.uint8)
    return c0, np.zeros_like(c0), np.full_like(c0, 255), last


FIXED = fixed_crops()


def batch(n):
    x = np.random.default_rng(1000 + n).integers(0, 256, (n, IMG_H, IMG_W, 3), dtype=np.uint8)
    x[0] = FIXED[0]
    if n >= 4:
        x[1], x[2], x[3] = FIXED[1], FIXED[2], FIXED[3]
    return x


def normalised(x_u8):
    """What the fp32 entry points are given: float32 of (2v - 255) / 255."""
    return ((2.0 * x_u8.astype(np.float64) - 255.0) / 255.0).astype(np.float32)


def sampled_images(n):
    if n <= 8:
        return list(range(n))
    rng = np.random.default_rng(n)
    return sorted({0, 1, 2, 3, n - 1} | set(int(i) for i in rng.choice(np.arange(4, n - 1), 2, replace=False)))


# ----------------------------------------------------------------------------- float64 oracle
def _patches(x64):
    xp = np.zeros((IMG_H + 6, IMG_W + 6, 3))
    xp[3:-3, 3:-3] = x64
    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(0, 1))[::2, ::2]          # [128, 64, 3, 7, 7]
    return np.ascontiguousarray(win.transpose(0, 1, 3, 4, 2)).reshape(MAP_H * MAP_W, K)


_WK = W.reshape(C, K).astype(np.float64).T
W1 = (_patches(np.ones((IMG_H, IMG_W, 3))) @ np.abs(_WK)).reshape(MAP_H, MAP_W, C)      # sum |w| over the taps inside the image
_ORACLE = {}


def conv_oracle(img):
    """One image [256, 128, 3] (uint8 crop, or the float32 the fp32 entry gets) -> float64 (acc, A, X1) of the module docstring,
    [128, 64, 64] / [128, 64, 1].  Computed once per image: the fixed crops come back in every batch."""
    key = (img.dtype.str, hash(img.tobytes()))
    if key not in _ORACLE:
        x = (2.0 * img.astype(np.float64) - 255.0) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)
        p = _patches(x)
        pa = np.abs(p)
        _ORACLE[key] = ((p @ _WK).reshape(MAP_H, MAP_W, C), (pa @ np.abs(_WK)).reshape(MAP_H, MAP_W, C),
                        pa.sum(1).reshape(MAP_H, MAP_W, 1))
    return _ORACLE[key]


def pool(v, pad=-np.inf, seams=(), seam_top=None):
    """MaxPool(3, 2, 1) of [h, w, c] with `pad` outside the image.  seams / seam_top: pooled rows whose TOP input row reads as
    seam_top - the model of a strip that starts there without the row kept from the tile above (the CPU checks that a wrong kernel
    would be seen; the oracle itself never passes them)."""
    h, w, c = v.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    vp = np.full((2 * ho + 2, 2 * wo + 2, c), pad, np.float64)
    vp[1:h + 1, 1:w + 1] = v
    out = np.full((ho, wo, c), -np.inf)
    for dy in range(3):
        for dx in range(3):
            t = vp[dy:dy + 2 * ho:2, dx:dx + 2 * wo:2]
            if dy == 0 and len(seams):
                t = t.copy()
                t[list(seams)] = seam_top
            out = np.maximum(out, t)
    return out


def epilogue(acc):
    return acc * SCALE.astype(np.float64) + SHIFT.astype(np.float64)


def bound(kind, acc, ab, x1, is_u8):
    """Per conv-map element, SAFETY included; kind: "0" mode 0, "2" mode 2, "1" fused mode 1, "5" unfused mode 1."""
    s = np.abs(SCALE.astype(np.float64))
    v = epilogue(acc)
    accs = np.abs(acc) * s
    epi = 4 * U * (accs + np.abs(SHIFT.astype(np.float64)))
    e_in = 2 * U * s * W1 if is_u8 else 0.0
    if kind == "0":
        b = s * K * U * ab + e_in + epi
    elif kind == "2" and is_u8:
        b = s * ((2.0 ** -33 + K * U * (1 + 2.0 ** -10)) * ab + 2.0 ** -47 * x1) + epi
    elif kind == "2":
        b = s * ((3 * 2.0 ** -22 + K * U * (1 + 2.0 ** -9)) * ab + 2.0 ** -36 * (W1 + x1)) + epi
    elif kind == "1":
        b = s * (2 * H16 + H16 * H16 + 2 * U + K * U) * ab + e_in + H16_ABS * x1 + H16 * accs + (H16 + U) * np.abs(v) + 2 * H16_ABS
    elif kind == "5":
        b = s * ((2 * H16 + H16 * H16 + K * U) * ab + H16_ABS * x1) + e_in + epi + H16 * np.abs(v) + H16_ABS
    else:
        raise ValueError(kind)
    return SAFETY * b


def f16_of(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


RATIOS = {}


def check(family, what, got, want, bnd):
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), "%s: non-finite output (NaN fill or overflow)" % what
    ratio = err / bnd
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio[worst]))
    print("RATIO %s %s worst err/bound %.4f (family so far %.4f)" % (family, what, ratio[worst], RATIOS[family]))
    assert (err <= bnd).all(), "%s: at %s got %r, float64 %r, bound %g" % (what, worst, got[worst], want[worst], bnd[worst])


def check_stem(family, what, got, x, kind, pooled=True):
    """got [n, 64, 32, 64] (or the conv map [n, 128, 64, 64]) against the oracle on the sampled images; every image finite.
    Returns {image: (oracle value, bound)}."""
    n = len(x)
    got = np.asarray(got)
    assert np.isfinite(got).all(), "%s: an element was left unwritten (NaN fill) or is not finite" % what
    res = {}
    for i in sampled_images(n):
        acc, ab, x1 = conv_oracle(x[i])
        v, b = epilogue(acc), bound(kind, acc, ab, x1, x.dtype == np.uint8)
        if pooled:
            v, b = pool(v), pool(b)
        check(family, "%s image %d" % (what, i), got[i], v, b)
        res[i] = (v, b)
    return res


# ----------------------------------------------------------------------------- CPU: the oracle and what it can see
def test_oracle_is_torch_conv_and_pool():
    import torch
    x = batch(5)[[0, 3, 4]]
    xt = torch.from_numpy((2.0 * x.astype(np.float64) - 255.0) / 255.0).permute(0, 3, 1, 2)
    conv = torch.nn.functional.conv2d(xt, torch.from_numpy(W.astype(np.float64)).permute(0, 3, 1, 2), None, 2, 3)
    conv = conv * torch.from_numpy(SCALE.astype(np.float64))[None, :, None, None] + torch.from_numpy(SHIFT.astype(np.float64))[None, :, None, None]
    pl = torch.nn.functional.max_pool2d(conv, 3, 2, 1)
    ab = torch.nn.functional.conv2d(xt.abs(), torch.from_numpy(np.abs(W.astype(np.float64))).permute(0, 3, 1, 2), None, 2, 3)
    for j, img in enumerate(x):
        acc, a, x1 = conv_oracle(img)
        np.testing.assert_allclose(epilogue(acc), conv[j].permute(1, 2, 0).numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(pool(epilogue(acc)), pl[j].permute(1, 2, 0).numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(a, ab[j].permute(1, 2, 0).numpy(), rtol=1e-12, atol=1e-12)
        assert (a <= W1 * (1 + 1e-12)).all() and (x1 <= K).all()           # |x| <= 1
    # odd sizes of the pool alone, against torch
    v = np.random.default_rng(3).normal(size=(5, 7, 8)) - 3.0
    want = torch.nn.functional.max_pool2d(torch.from_numpy(v).permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0).numpy()
    np.testing.assert_array_equal(pool(v), want)


def test_sampled_images_equal_dense():
    """The sampled-image path (what the large batches are held to) is the dense one restricted to those images, bit for bit."""
    n = 12
    x = batch(n)
    imgs = sampled_images(n)
    assert imgs[:4] == [0, 1, 2, 3] and imgs[-1] == n - 1 and 7 == len(imgs) < n
    xn = (2.0 * x.astype(np.float64) - 255.0) / 255.0
    dense = np.stack([(_patches(xi) @ _WK).reshape(MAP_H, MAP_W, C) for xi in xn])
    for i in imgs:
        np.testing.assert_array_equal(conv_oracle(x[i])[0], dense[i])
    assert sampled_images(5) == [0, 1, 2, 3, 4] and sampled_images(214)[-1] == 213


def test_zero_padded_or_seamed_pool_would_fail():
    """A pool that pads with 0, or a strip whose first tile starts from 0 instead of the row of the tile above, is off by more than
    every bound at image-border elements and at interior elements of every seam row - for the fixed crops and a random one, for every
    strip count, in every mode.  A seam that merely loses the row above (starts from -inf) is smaller but still seen on noise."""
    x = batch(5)
    for i in range(5):
        acc, ab, x1 = conv_oracle(x[i])
        v = epilogue(acc)
        good = pool(v)
        assert (v.max(axis=(0, 1)) < 0).sum() >= 16, "whole maps must be negative"
        for kind in ("0", "2", "1", "5"):
            b = pool(bound(kind, acc, ab, x1, True))
            bad = np.abs(pool(v, pad=0.0) - good) > b
            assert bad[0, 1:].any() and bad[1:, 0].any() and bad[0, 0].any(), "border row / column / corner of a 0-padded pool"
            assert not bad[1:, 1:].any()                   # ... and only there: row 127 and column 63 never reach the padding
            for s in SPLIT_STRIPS[:-1] + (8,):             # (8: launch_stem_f32's pooled strips of 8 tiles)
                seams = split_seams(s)
                from_zero = np.abs(pool(v, seams=seams, seam_top=0.0) - good) > b
                assert all(from_zero[t, 1:].any() for t in seams), "a seam row that starts from 0: %d strips" % s
                assert not np.delete(from_zero, seams, axis=0).any()
                if i == 4 and kind in ("0", "2"):
                    lost = np.abs(pool(v, seams=seams, seam_top=-np.inf) - good) > b
                    assert all(lost[t, 1:].any() for t in seams), "a seam row without the row above: %d strips" % s


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    blob, manifest, _ = weights.pack_seres18(synth.seres18_state_dict(0))
    e.load_seres18(blob, manifest)
    e.set_precision(0)
    return e


def stem(eng, form, x):
    return eng.debug_stem(form, x, W, SCALE, SHIFT)


@pytest.fixture(scope="module")
def split_image0(eng):
    """Image 0 alone (64 strips): what image 0 of every other batch must equal bit for bit, per input type."""
    x = batch(1)
    return {"u8": stem(eng, 2, x), "f32": stem(eng, 2, normalised(x))}


# ----------------------------------------------------------------------------- stem_split (form 2)
def check_packed(pk, v32, what):
    """[xh | xl'] is the split of the kernel's own fp32 value, bit for bit."""
    v = v32.reshape(-1, C)
    yh = v.astype(np.float16)
    yl = ((v - yh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    np.testing.assert_array_equal(pk[:, :C], yh.view(np.uint16), err_msg="%s: xh" % what)
    np.testing.assert_array_equal(pk[:, C:], yl.view(np.uint16), err_msg="%s: xl'" % what)


@gpu
@pytest.mark.parametrize("n,strips", list(zip(SPLIT_N, SPLIT_STRIPS)), ids=["n%d-s%d" % p for p in zip(SPLIT_N, SPLIT_STRIPS)])
def test_stem_split(eng, split_image0, n, strips):
    """launch_stem_split at the smallest batch of every strip count, uint8 and fp32 input: the oracle, the packed form, image 0's bits
    at every strip count, and the two input types against each other (the sum of their bounds)."""
    assert split_strips(n) == strips            # the restated rule (module docstring): the launcher does not report its choice
    x = batch(n)
    outs = {}
    for name, xin in (("u8", x), ("f32", normalised(x))):
        what = "stem_split %s n=%d (%d strips)" % (name, n, strips)
        out, pk = stem(eng, 2, xin)
        ref = check_stem("stem_split-" + name, what, out, xin, "2")
        check_packed(pk, out, what)
        np.testing.assert_array_equal(out[0], split_image0[name][0][0], err_msg="%s: image 0 differs from the 64-strip launch" % what)
        np.testing.assert_array_equal(pk[:2048], split_image0[name][1], err_msg="%s: packed image 0" % what)
        recon = (f16_of(pk[:, :C]) + f16_of(pk[:, C:]) / 2048.0).reshape(n, 64, 32, C)
        for i, (v, b) in ref.items():
            check("stem_split-packed", "%s packed image %d" % (what, i), recon[i], v, b + 2.0 ** -22 * (np.abs(v) + b) + 2.0 ** -36)
        outs[name] = (out, ref)
    for i in outs["u8"][1]:
        bu, bf = outs["u8"][1][i][1], outs["f32"][1][i][1]
        d = np.abs(outs["u8"][0][i].astype(np.float64) - outs["f32"][0][i])
        assert (d <= bu + bf).all(), "n=%d image %d: uint8 and fp32 entry differ by %g" % (n, i, d.max())


@gpu
def test_stem_split_reports_an_input_beyond_f16(eng):
    """stem_split_kernel<false> takes the fault word: an fp32 input f16 cannot hold makes the call fail with REID_ERR_STATE, clear_fault
    resets it, and the next call is clean."""
    x = normalised(batch(1))
    x[0, 100, 50, 1] = 70000.0
    with pytest.raises(_ffi.ReidHipError) as ei:
        stem(eng, 2, x)
    assert ei.value.status == -3
    assert eng.fault_bits() & 1
    eng.clear_fault()
    assert eng.fault_bits() == 0
    x[0, 100, 50, 1] = 1.0
    check_stem("stem_split-f32", "after clear_fault", stem(eng, 2, x)[0], x, "2")


# ----------------------------------------------------------------------------- stem_f32 (forms 0 and 1)
@gpu
@pytest.mark.parametrize("n", F32_N)
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_stem_f32(eng, kind, n):
    """launch_stem_f32 unpooled (1 / 2 / 4 / 8 / 16 tiles per block) and pooled (8, 16 at n = 128) against the oracle; the pooled
    launch equals the max-pool kernel on the unpooled map bit for bit (module docstring)."""
    x = batch(n) if kind == "u8" else normalised(batch(n))
    what = "stem_f32 %s n=%d" % (kind, n)
    conv = stem(eng, 0, x)[0]
    check_stem("stem_f32-map-" + kind, what + " unpooled", conv, x, "0", pooled=False)
    pooled = stem(eng, 1, x)[0]
    check_stem("stem_f32-pool-" + kind, what + " pooled", pooled, x, "0")
    np.testing.assert_array_equal(pooled, eng.debug_maxpool(conv), err_msg=what + ": fused pool against maxpool3s2 of the map")


# ----------------------------------------------------------------------------- mode 1 (forms 3, 4, 5)
@gpu
@pytest.mark.parametrize("n", (1, 6, 128))
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_stem_f16(eng, kind, n):
    x = batch(n) if kind == "u8" else normalised(batch(n))
    what = "stem_f16 %s n=%d" % (kind, n)
    fused = stem(eng, 4, x)[1]
    check_stem("stem_pool_f16-" + kind, what + " prep + fused", f16_of(fused), x, "1")
    if kind == "u8":
        direct = stem(eng, 3, x)[1]
        np.testing.assert_array_equal(direct, fused, err_msg=what + ": straight from uint8 against prep + fused")
    unfused = stem(eng, 5, x)[1]
    check_stem("stem_gemm16-" + kind, what + " prep + GEMM + pool", f16_of(unfused), x, "5")


# ----------------------------------------------------------------------------- generic GEMM stem (form 6)
@gpu
@pytest.mark.parametrize("n", (1, 6))
def test_stem_generic_gemm(eng, n):
    """conv_gemm(A_STEM_U8 / A_STEM_F32) + maxpool3s2 at precisions 0 and 2: the exact-fp32 GEMM both times, the same bits."""
    for kind, x in (("u8", batch(n)), ("f32", normalised(batch(n)))):
        outs = []
        for prec in (0, 2):
            eng.set_precision(prec)
            try:
                outs.append(stem(eng, 6, x)[0])
            finally:
                eng.set_precision(0)
            check_stem("stem_gemm32-" + kind, "A_STEM %s n=%d precision %d" % (kind, n, prec), outs[-1], x, "0")
        np.testing.assert_array_equal(outs[0], outs[1])


# ----------------------------------------------------------------------------- max-pool alone
POOL_SHAPES = [(1, 2, 2, 4), (2, 5, 7, 8), (1, 128, 64, 64), (3, 9, 6, 64)]


@gpu
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["x".join(map(str, s)) for s in POOL_SHAPES])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_maxpool_alone(eng, f16, shape):
    """Negative inputs (a 0-padded pool would return 0 along the border), exact against the float64 oracle.  The f16 kernel moves
    eight channels at a time: its launcher refuses c = 4 instead of leaving the output unwritten."""
    n, h, w, c = shape
    x = (-np.abs(np.random.default_rng(h * w + c).normal(size=shape)) - 0.25).astype(np.float16 if f16 else np.float32)
    if f16 and c % 8:
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.debug_maxpool(x.view(np.uint16))
        assert ei.value.status == -1
        return
    got = eng.debug_maxpool(x.view(np.uint16) if f16 else x)
    got = f16_of(got) if f16 else got.astype(np.float64)
    want = np.stack([pool(xi.astype(np.float64)) for xi in x])
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert (want < 0).all()


# ----------------------------------------------------------------------------- resize
RESIZE_HW = [(1, 1), (1, 7), (9, 1), (2, 2), (3, 300), (256, 128), (400, 160), (41, 13), (257, 129)]
FRAME_H, FRAME_W = 480, 640
# top-left corner of each window in the frame: together they touch all four borders and all four corners
RESIZE_YX = [(0, 0), (0, FRAME_W - 7), (FRAME_H - 9, 0), (FRAME_H - 2, FRAME_W - 2), (10, FRAME_W - 300), (FRAME_H - 256, 100), (0, 200),
             (200, 0), (FRAME_H - 257, FRAME_W - 129)]


def resize_inputs():
    frame = np.random.default_rng(99).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    crops = [np.ascontiguousarray(frame[y:y + h, x:x + w]) for (h, w), (y, x) in zip(RESIZE_HW, RESIZE_YX)]
    return frame, crops


def _taps64(dst, src):
    c = (np.arange(dst) + 0.5) * (src / dst) - 0.5
    s = np.floor(c).astype(np.int64)
    f = c - s
    lo, hi = s < 0, s >= src - 1
    s[lo], f[lo] = 0, 0.0
    s[hi], f[hi] = src - 1, 0.0
    return c, s, f


def _local_max(d, iy, ix, ry, rx):
    """max of d[iy + a, ix + b] over a in ry, b in rx (indices clamped), [len(iy), len(ix), 3]; an empty d (1-pixel crops) gives 0."""
    out = np.zeros((len(iy), len(ix), 3))
    if d.shape[0] == 0 or d.shape[1] == 0:
        return out
    for a in ry:
        for b in rx:
            out = np.maximum(out, d[np.clip(iy + a, 0, d.shape[0] - 1)][:, np.clip(ix + b, 0, d.shape[1] - 1)])
    return out


def resize64(crop):
    """float64 restatement of the crop preprocessing and the module docstring's bound br, both [256, 128, 3]."""
    p = crop.astype(np.float64) / 255.0
    h, w = p.shape[:2]
    cx, sx, fx = _taps64(IMG_W, w)
    cy, sy, fy = _taps64(IMG_H, h)
    x1, y1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    rows = p[:, sx] * (1.0 - fx)[None, :, None] + p[:, x1] * fx[None, :, None]
    v = rows[sy] * (1.0 - fy)[:, None, None] + rows[y1] * fy[:, None, None]
    dx = _local_max(np.abs(np.diff(p, axis=1)), sy, sx, (-1, 0, 1, 2), (-1, 0, 1))
    dy = _local_max(np.abs(np.diff(p, axis=0)), sy, sx, (-1, 0, 1), (-1, 0, 1, 2))
    b = 2.0 * (U * (np.abs(cx) + 1.0)[None, :, None] * dx + U * (np.abs(cy) + 1.0)[:, None, None] * dy + 10 * U)
    return (v - 0.5) / 0.5, SAFETY * b


def test_resize_restatement_bounds_the_fp32_oracle():
    """oracle.matching.preprocess (fp32, what the kernel must equal bit for bit) is within br of the float64 restatement: the bound
    holds for the arithmetic the kernel claims to do, on every crop shape of the GPU test."""
    from oracle import matching
    _, crops = resize_inputs()
    worst = 0.0
    for crop in crops:
        want, b = resize64(crop)
        got = matching.preprocess([crop])[0].transpose(1, 2, 0).astype(np.float64)
        assert (np.abs(got - want) <= b).all(), crop.shape
        worst = max(worst, float((np.abs(got - want) / b).max()))
    assert worst > 0.0                # the two are different computations
    ident = matching.preprocess([crops[5]])[0].transpose(1, 2, 0)
    np.testing.assert_array_equal(ident, ((crops[5].astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5))


@gpu
def test_resize_on_device(eng):
    """resize_norm_kernel on ragged packed crops and on the same crops as windows of a frame (pitch 640, boxes on all four borders):
    bit equality with the numpy oracle and between the two forms, and the float64 bound.  (This test found the kernel's lerps fused
    into FMAs: 11.5 % of a 1 x 7 crop's outputs were 1 ulp off the oracle until the kernel was built with fp contract(off).)"""
    from oracle import matching
    frame, crops = resize_inputs()
    packed = np.concatenate([c.reshape(-1) for c in crops])
    sizes = np.array([c.size for c in crops], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    hw = np.array(RESIZE_HW, np.int32)
    got = eng.debug_resize_norm(packed, offsets, hw)
    assert np.isfinite(got).all()
    want = matching.preprocess(crops).transpose(0, 2, 3, 1)
    for i, crop in enumerate(crops):
        np.testing.assert_array_equal(got[i], want[i], err_msg="crop %s against oracle.matching.preprocess" % (crop.shape,))
        v, b = resize64(crop)
        check("resize", "crop %dx%d" % crop.shape[:2], got[i], v, b)
    f_off = np.array([(y * FRAME_W + x) * 3 for y, x in RESIZE_YX], np.int64)
    from_frame = eng.debug_resize_norm(frame, f_off, hw, pitch=FRAME_W)
    np.testing.assert_array_equal(from_frame, got, err_msg="windows of a frame against packed crops")
