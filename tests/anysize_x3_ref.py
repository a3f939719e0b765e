"""numpy restatement of the fp32-class convolution of the any-size forward (csrc/anysize_x3.hip), and the inputs its tests share.

Arithmetic: xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11) - both kept with f16's subnormals -, weights wq = f16(wh 2^11),
wh = f16_rn(w), wl' = f16_rn((w - wh) 2^11); an output element is 2^-11 (sum_k xh wq + xl' wh + xh wl').  Here the parts are np.float16
and the sums float64, so `restate` is that value without the kernel's fp32 accumulation error; on the EXACT family every term is a
multiple of 0.25 and the sum of magnitudes stays below 2^24 quarters, so fp32 accumulation is exact in any order and the kernel has to
return float32(restate) bit for bit - which a dropped product, a wrong tap, a swapped part or a lost row cannot do.  The SMALL family
(|x| ~ 2^-15) puts xh near and xl' deep inside f16's subnormal range: flushing either part is far outside the float64 bound."""
import numpy as np

# name: (cin, cout, r, stride, h, w, n) - the smallest shapes at which each code path of the kernel can still go wrong
GEOMS = {
    "l1": (64, 64, 3, 1, 7, 5, 3),         # one ragged tile, rows crossing image borders
    "l1big": (64, 64, 3, 1, 23, 11, 2),    # several tiles and a ragged last one (M = 506)
    "l2s": (64, 128, 3, 2, 9, 7, 3),       # odd map, stride 2
    "l2d": (64, 128, 1, 2, 9, 7, 3),       # 1x1 stride 2, K = 64
    "l2": (128, 128, 3, 1, 5, 4, 3),
    "l3s": (128, 256, 3, 2, 5, 4, 3),
    "l3d": (128, 256, 1, 2, 5, 4, 3),
    "l3": (256, 256, 3, 1, 3, 2, 5),
    "l4a": (256, 512, 3, 1, 3, 2, 5),
    "l4d": (256, 512, 1, 1, 3, 2, 5),
    "l4": (512, 512, 3, 1, 2, 2, 5),       # K = 4608; at 2 x 2 most taps are padding
}
F16_MIN_NORMAL = 2.0 ** -14


def pad_of(r):
    return 1 if r == 3 else 0


def out_hw(name):
    cin, cout, r, stride, h, w, n = GEOMS[name]
    p = pad_of(r)
    return (h + 2 * p - r) // stride + 1, (w + 2 * p - r) // stride + 1


def exact_operands(name, seed):
    """x = (+-1 + l 2^-13) kept with probability 0.25 (0 otherwise), w the same with every weight kept, l in {-1, 0, 1}."""
    cin, cout, r, stride, h, w, n = GEOMS[name]
    rng = np.random.default_rng(seed)

    def draw(shape):
        return (rng.choice([-1.0, 1.0], shape) + rng.integers(-1, 2, shape) * 2.0 ** -13).astype(np.float32)
    x = draw((n, h, w, cin)) * (rng.random((n, h, w, cin)) < 0.25)
    return x.astype(np.float32), draw((cout, r, r, cin))


def small_operands(name, seed):
    cin, cout, r, stride, h, w, n = GEOMS[name]
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, h, w, cin)) * 2.0 ** -15).astype(np.float32)
    return x, rng.normal(0, 0.05, (cout, r, r, cin)).astype(np.float32)


def random_operands(name, seed):
    cin, cout, r, stride, h, w, n = GEOMS[name]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    wt = rng.normal(0, np.sqrt(2.0 / (r * r * cin)), (cout, r, r, cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(size=cout).astype(np.float32)
    ho, wo = out_hw(name)
    res = rng.normal(size=(n, ho, wo, cout)).astype(np.float32)
    return x, wt, scale, shift, res


def _flush(part):
    return np.where(np.abs(part) < F16_MIN_NORMAL, 0.0, part)


def split(v, flush_hi=False, flush_lo=False):
    """fp32 -> (hi, lo') as float64 arrays holding f16 values; flush_*: that part without f16's subnormals (the mutation)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    return (_flush(hi) if flush_hi else hi), (_flush(lo) if flush_lo else lo)


def im2col(x, r, stride):
    """[n, h, w, c] -> [n ho wo, r r c], k = (tap, channel), zero padding."""
    n, h, w, c = x.shape
    p = pad_of(r)
    xp = np.zeros((n, h + 2 * p, w + 2 * p, c), x.dtype)
    xp[:, p:p + h, p:p + w] = x
    ho, wo = (h + 2 * p - r) // stride + 1, (w + 2 * p - r) // stride + 1
    cols = [xp[:, ty:ty + (ho - 1) * stride + 1:stride, tx:tx + (wo - 1) * stride + 1:stride] for ty in range(r) for tx in range(r)]
    return np.stack(cols, 3).reshape(n * ho * wo, r * r * c)


def restate(x, w, stride, drop=None, flush_hi=False, flush_lo=False):
    """(value, magnitude): the three-product value 2^-11 (xh.wq + xl'.wh + xh.wl') in float64 on every output element [m, cout], and the sum
    of the terms' magnitudes on the accumulator's scale (before the 2^-11).  drop: "lh" leaves xl'.wh out, "hl" xh.wl' (mutations)."""
    r = w.shape[1]
    xh, xl = split(x, flush_hi, flush_lo)
    wh, wl = split(w)
    wq = (wh.astype(np.float32) * np.float32(2048.0)).astype(np.float16).astype(np.float64)
    ah, al = im2col(xh, r, stride), im2col(xl, r, stride)
    bq, bh, bl = (t.reshape(w.shape[0], -1).T for t in (wq, wh, wl))
    acc = ah @ bq
    mag = np.abs(ah) @ np.abs(bq)
    if drop != "lh":
        acc = acc + al @ bh
        mag = mag + np.abs(al) @ np.abs(bh)
    if drop != "hl":
        acc = acc + ah @ bl
        mag = mag + np.abs(ah) @ np.abs(bl)
    return acc * 2.0 ** -11, mag
