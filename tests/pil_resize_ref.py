"""Numpy restatement of Pillow's 8-bit bilinear resize (Resample.c) and of ToTensor + Normalize, without a PIL import: the yardstick of
tests/test_pil_resize_host.py and tests/test_gpu_pil_resize.py.

The evaluation script's transform is transforms.Resize((H, W)) on an RGB PIL image, i.e. img.resize((W, H), BILINEAR) with
reducing_gap=None, then ToTensor and Normalize(mean, std) (reid/data_transforms.py:56-127); the mirrored view flips the resized image
(:130-209).  Pillow's 8-bit path makes two passes, the horizontal one first into a uint8 image, the vertical one on that rounded image.
Per axis, in_size -> out_size, every real operation an IEEE double (Python floats are doubles; nothing here can be contracted):

    scale = in_size / out_size;  fs = max(scale, 1.0);  support = 1.0 * fs;  ksize = 2 * ceil(support) + 1
    center = (xx + 0.5) * scale
    xmin = max(0, (int)(center - support + 0.5));  xmax = min(in_size, (int)(center + support + 0.5)) - xmin
    w[x] = tri(((x + xmin) - center + 0.5) * (1.0 / fs)),  tri(a) = 1 - |a| if |a| < 1 else 0
    ww = w[0] + w[1] + ... in that order;  w[x] /= ww if ww != 0
    k[x] = (int)(0.5 + w[x] * (1 << 22))            ((int)(-0.5 + ...) for a negative weight)
    out[xx] = clamp(((1 << 21) + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)

The keyword switches of coeffs() and resize_u8() each break ONE of these rules; the tests use them to show that the fixture tells every
rule from its nearest wrong reading.  Their defaults are Pillow's arithmetic.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # Resample.c: coefficients are fixed point with 22 fractional bits
IMAGENET_MEAN_STD = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)

# the sources and output sizes the oracle was checked on against Image.resize (tests/test_pil_resize_host.py does it again where PIL is
# importable), and the GPU harness test's ragged call
SOURCES = ((128, 64), (256, 128), (300, 117), (257, 129), (511, 255), (90, 200), (1, 1), (2, 3), (700, 301), (64, 32), (1031, 517), (256, 64),
           (100, 128))
OUT_SIZES = ((256, 128), (448, 224), (224, 224))


def coeffs(in_size, out_size, widen=True, renorm=True):
    """-> k int32 [out_size][ksize] (zero beyond xmax), bounds int32 [out_size][2] = (xmin, xmax), ksize."""
    scale = in_size / out_size
    fs = max(scale, 1.0) if widen else 1.0
    support = 1.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))          # int() truncates toward zero, as the C cast
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = ((x + xmin) - center + 0.5) * ss
            a = -a if a < 0.0 else a
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if (ww != 0.0 and renorm) else w[x]
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds, ksize


def _pass(img, axis, out_size, rounding=True, exact=False, **kw):
    """One pass along `axis` (0 vertical, 1 horizontal) of an [h][w][c] image.  exact: the unrounded value as float64."""
    k, bounds, _ = coeffs(img.shape[axis], out_size, **kw)
    src = np.moveaxis(img, axis, 0)
    out = np.empty((out_size,) + src.shape[1:], np.float64 if exact else np.uint8)
    half = (1 << (PRECISION_BITS - 1)) if rounding else 0
    for xx in range(out_size):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        kk = k[xx, :xmax].reshape((xmax,) + (1,) * (src.ndim - 1))
        if exact or src.dtype != np.uint8:
            acc = (src[xmin:xmin + xmax].astype(np.float64) * kk).sum(0) / (1 << PRECISION_BITS)
            out[xx] = acc if exact else np.clip(np.floor(acc + (0.5 if rounding else 0.0)), 0, 255)
        else:
            acc = half + (src[xmin:xmin + xmax].astype(np.int64) * kk.astype(np.int64)).sum(0)
            out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, out_h, out_w, vertical_first=False, round_between=True, widen=True, rounding=True, renorm=True):
    """img uint8 [h][w][c] -> uint8 [out_h][out_w][c], Image.resize((out_w, out_h), BILINEAR) with every switch at its default."""
    img = np.ascontiguousarray(img, np.uint8)
    kw = dict(widen=widen, renorm=renorm)
    order = ((0, out_h), (1, out_w)) if vertical_first else ((1, out_w), (0, out_h))
    first = _pass(img, order[0][0], order[0][1], rounding=rounding, exact=not round_between, **kw)
    return np.ascontiguousarray(_pass(first, order[1][0], order[1][1], rounding=rounding, **kw))


def norm_table(mean_std=IMAGENET_MEAN_STD):
    """float32 [3][256]: (v / 255 - mean) / std in float32 with two true divisions - torch's to(float32).div(255).sub_(mean).div_(std)."""
    ms = np.asarray(mean_std, np.float32).reshape(2, 3)
    v = np.arange(256, dtype=np.float32)[None, :] / np.float32(255.0)
    return ((v - ms[0][:, None]) / ms[1][:, None]).astype(np.float32)


def to_float(u8, mean_std=IMAGENET_MEAN_STD):
    """uint8 [h][w][3] -> float32 [3][h][w], ToTensor + Normalize."""
    t = norm_table(mean_std)
    return np.stack([t[c][u8[:, :, c]] for c in range(3)])


def preprocess(images, out_h, out_w, mean_std=IMAGENET_MEAN_STD):
    """list of uint8 [h][w][3] -> float32 [n][3][out_h][out_w]: what the evaluation script's transform hands the model."""
    return np.stack([to_float(resize_u8(im, out_h, out_w), mean_std) for im in images]) if len(images) else np.zeros((0, 3, out_h, out_w), np.float32)


def formula_image(h, w, salt=0):
    """The stated integer formula of the large fixture cases: no RNG stream.  Row 0 and column 0 are 0, the last row and column 255
    (saturated borders), the rest a hash of (y, x, c)."""
    y = np.arange(h, dtype=np.int64)[:, None, None]
    x = np.arange(w, dtype=np.int64)[None, :, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    v = ((y * 131 + x * 71 + c * 29 + salt * 17) * (y + 3 * x + 7 * c + 11) + ((y * x) >> 2)) % 256
    v = np.broadcast_to(v, (h, w, 3)).copy()
    v[0, :, :] = 0
    v[:, 0, :] = 0
    v[h - 1, :, :] = 255
    v[:, w - 1, :] = 255
    return v.astype(np.uint8)
