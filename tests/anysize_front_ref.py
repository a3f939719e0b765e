"""float64 restatement of the front end of the any-size ResNet18-IBN-SE forward - cv2-style bilinear resize -> Normalize -> conv 7x7 s2 p3
-> folded BatchNorm (no ReLU) -> MaxPool2d(3, 2, 1) - for any (H, W), with a per-element error bound for what the device computes in fp32
(any_front_kernel of csrc/anysize_front.hip and the three launches it replaces: both claim the same arithmetic).

The bound is put together from the pieces tests/test_gpu_frontend.py derives, imported from there (its docstring has the derivations):
  * resize: `_taps64`, `_local_max` and the formula of `resize64`, br = SAFETY (u (|cx| + 1) Dx + u (|cy| + 1) Dy + 10 u) / std.  resize64
    itself is written for 256 x 128 and 0.5 / 0.5 (its factor 2 is 1 / std); `resized` below is the same computation with the size, mean and
    std as arguments - at (256, 128), 0.5 / 0.5 the two agree exactly (tests/test_anysize_front_host.py).  With another std the division
    rounds once more: + SAFETY u |value|.
  * convolution and epilogue: `bound("0", acc, A, X1, False)` - K fp32 accumulations of exact fp32 products and the epilogue's roundings
    for an fp32 input.  The function reads its module's SCALE and SHIFT, so `conv_bound` calls it with the caller's in their place.
  * the input's own error reaches an output through |w|: + |scale| conv(br, |w|).
  * pooling: `pool` for values and bounds alike: max is 1-Lipschitz in the sup norm over its window.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_frontend as fe  # noqa: E402

U, SAFETY, K = fe.U, fe.SAFETY, fe.K
# the sizes of the GPU test: smallest map; odd H1 / H2; DeepSORT's crop; the fixture's size; wide, odd; tall (several bands, a ragged last
# one); widest LDS row and nine column tiles (one crop only); and (33, 49), whose W1 = 25 and W2 = 13 are odd as well (47 gives W1 = 24)
SIZES = ((32, 32), (33, 47), (128, 64), (96, 72), (57, 131), (200, 40), (512, 512), (33, 49))
SOURCES = ((1, 1), (9, 300), (300, 200))
OTHER_MEAN_STD = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def maps(h, w):
    h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h1, w1, (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1


def crops(seed=5):
    """One uint8 crop per SOURCES shape: noise, so that neighbouring pixels differ by much (the resize bound is not small by luck)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCES]


def stem_of(sd):
    """(w [64, 7, 7, 3], packed [64, 192], scale [64], shift [64]) of a ResNet18-IBN-SE state dict."""
    from reid_amd import weights
    w = np.asarray(sd["conv0.weight"], np.float32)
    scale, shift = weights.fold_bn(sd, "bn0")
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1)), weights.stem_pack(w), scale, shift


def _mean_std(mean_std):
    ms = np.asarray(((0.5,) * 3, (0.5,) * 3) if mean_std is None else mean_std, np.float32).astype(np.float64)
    return ms[0], ms[1]


def resized(crop, h, w, mean_std=None, taps_size=None):
    """(value, bound) [h, w, 3] of the resize + Normalize.  taps_size: the (H, W) the taps are computed for - a mutation only."""
    mean, std = _mean_std(mean_std)
    p = crop.astype(np.float64) / 255.0
    sh, sw = p.shape[:2]
    th, tw = (h, w) if taps_size is None else taps_size
    cx, sx, fx = (a[np.arange(w) % tw] for a in fe._taps64(tw, sw))
    cy, sy, fy = (a[np.arange(h) % th] for a in fe._taps64(th, sh))
    x1, y1 = np.minimum(sx + 1, sw - 1), np.minimum(sy + 1, sh - 1)
    rows = p[:, sx] * (1.0 - fx)[None, :, None] + p[:, x1] * fx[None, :, None]
    v = rows[sy] * (1.0 - fy)[:, None, None] + rows[y1] * fy[:, None, None]
    dx = fe._local_max(np.abs(np.diff(p, axis=1)), sy, sx, (-1, 0, 1, 2), (-1, 0, 1))
    dy = fe._local_max(np.abs(np.diff(p, axis=0)), sy, sx, (-1, 0, 1), (-1, 0, 1, 2))
    out = (v - mean) / std
    b = (U * (np.abs(cx) + 1.0)[None, :, None] * dx + U * (np.abs(cy) + 1.0)[:, None, None] * dy + 10 * U) / std + U * np.abs(out)
    return out, SAFETY * b


def patches(x):
    """[h, w, 3] -> [H1, W1, 147]: the 7 x 7 windows at stride 2 with 3 zero pixels around, in (r, s, c) order."""
    h, w = x.shape[:2]
    h1, w1 = maps(h, w)[:2]
    xp = np.zeros((2 * h1 + 5, 2 * w1 + 5, 3))
    xp[3:3 + h, 3:3 + w] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(0, 1))[::2, ::2][:h1, :w1]
    return np.ascontiguousarray(win.transpose(0, 1, 3, 4, 2)).reshape(h1, w1, K)


def conv_bound(acc, ab, x1, scale, shift):
    """test_gpu_frontend.bound for mode 0 and an fp32 input, with `scale` / `shift` where that module keeps its own."""
    old = fe.SCALE, fe.SHIFT
    fe.SCALE, fe.SHIFT = np.asarray(scale, np.float32), np.asarray(shift, np.float32)
    try:
        return fe.bound("0", acc, ab, x1, False)
    finally:
        fe.SCALE, fe.SHIFT = old


def front64(crop, h, w, wgt, scale, shift, mean_std=None, pad=-np.inf, drop_last=False, taps_size=None):
    """(pooled value, pooled bound) [H2, W2, 64] in float64.  wgt [64, 7, 7, 3].  The last three arguments are the mutations of
    tests/test_anysize_front_host.py: another pool padding, the last stem row / column left out of the pool when H1 / W1 is odd, the taps
    of another size."""
    x, bx = resized(crop, h, w, mean_std, taps_size)
    wk = wgt.reshape(64, K).astype(np.float64).T
    p = patches(x)
    s = scale.astype(np.float64)
    acc = p @ wk
    v = acc * s + shift.astype(np.float64)
    b = conv_bound(acc, np.abs(p) @ np.abs(wk), np.abs(p).sum(-1, keepdims=True), scale, shift) + np.abs(s) * (patches(bx) @ np.abs(wk))
    if drop_last:
        h1, w1 = v.shape[:2]
        v = v.copy()
        if h1 % 2:
            v[h1 - 1] = -np.inf
        if w1 % 2:
            v[:, w1 - 1] = -np.inf
    return fe.pool(v, pad=pad), fe.pool(b)
