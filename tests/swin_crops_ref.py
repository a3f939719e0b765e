"""numpy restatement of the front end of the Swin uint8 entry points (csrc/swin_crops.hip), shared by tests/test_swin_crops_host.py and
tests/test_gpu_swin_crops.py.

``preprocess`` is the fp32 two-step path: what a caller of reid_swin_embed_f32_nchw does on the host, and what the fused kernel must
reproduce bit for bit - / 255, oracle.matching.resize_bilinear (bit-equal to the ResNet resize kernel), (x - mean) / std, CHW.

``front64`` is the float64 restatement of the whole kernel (resize, normalise, the stem's 2x2 stride-2 convolution) with a bound per
element, derived from the fp32 error model and not from observed numbers.  u = 2^-24.

  resize      tests/test_gpu_frontend.py's construction: the kernel rounds a tap coordinate c to fp32, |c' - c| <= u |c| <= u src; the
              interpolant is piecewise linear with slope at most Dx (Dy), the largest difference of horizontally (vertically) adjacent
              pixels / 255 among the taps' neighbours.  The chain / 255 (u), 1 - f (u), two products and a sum per lerp (3u each, values
              <= 1) is 9u:        e_v = u (|cx| + 1) Dx + u (|cy| + 1) Dy + 9u.
  normalise   t = fl(v - mean): |t| <= 1, one rounding, e_t = e_v + u (the frontend test's 10u); x = fl(t / std), a correctly rounded
              division: e_x = e_t / std + u |x|.  mean and std are the same fp32 numbers on both sides.
  convolve    c1 = bias + sum_k w_k x_k, 12 terms, one rounding each (FMA chain): the inputs' errors pass through as sum_k |w_k| e_x,k
              and the chain adds g_12 (|bias| + sum_k |w_k x_k|), g_12 = 12u / (1 - 12u)  (Higham 3.1).
  Both bounds are multiplied by SAFETY = 2 (the frontend test's factor) for the second-order terms dropped above.
"""
import numpy as np

from oracle import matching

U = 2.0 ** -24
SAFETY = 2.0
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], np.float32)      # reid/data_transforms.py:64
IMAGENET_STD = np.array([0.229, 0.224, 0.225], np.float32)
OTHER_MEAN_STD = np.array([0.5, 0.25, 0.625, 0.5, 0.1875, 0.3], np.float32)   # a non-default mean_std6: every channel differs

FRAME_H, FRAME_W = 480, 640
# (h, w) of each window and its top-left (y, x) in the frame: 1-pixel and 2-pixel windows (taps and clamps), the identity, one pixel off
# it both ways (h / w order), an upscale, two downscales; together the boxes touch all four borders of the frame
CROP_HW = [(1, 1), (1, 7), (7, 1), (2, 2), (224, 224), (223, 225), (37, 91), (448, 224), (470, 300)]
CROP_YX = [(0, 0), (0, FRAME_W - 7), (FRAME_H - 7, 0), (FRAME_H - 2, FRAME_W - 2), (100, 200), (FRAME_H - 223, FRAME_W - 225), (0, 300),
           (FRAME_H - 448, 0), (5, FRAME_W - 300)]


def crop_set():
    """(frame uint8 [480, 640, 3], crops as contiguous copies, boxes int32 [9, 4] as x1, y1, x2, y2)."""
    frame = np.random.default_rng(99).integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8)
    crops = [np.ascontiguousarray(frame[y:y + h, x:x + w]) for (h, w), (y, x) in zip(CROP_HW, CROP_YX)]
    boxes = np.array([(x, y, x + w, y + h) for (h, w), (y, x) in zip(CROP_HW, CROP_YX)], np.int32)
    return frame, crops, boxes


def packed(crops):
    """(bytes, offsets int64, hw int32 [n, 2]) of crops laid one after the other."""
    sizes = np.array([c.size for c in crops], np.int64)
    return (np.concatenate([c.reshape(-1) for c in crops]), np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64),
            np.array([c.shape[:2] for c in crops], np.int32))


def preprocess(crops, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [h_i, w_i, 3] crops -> float32 [n, 3, H, W], size = (H, W): every operation a separate fp32 rounding."""
    H, W = size
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    out = []
    for im in crops:
        x = matching.resize_bilinear(np.asarray(im).astype(np.float32) / np.float32(255.0), (W, H))
        x = (x - mean) / std
        out.append(np.transpose(x, (2, 0, 1)))
    return np.stack(out, 0).astype(np.float32)


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


def preprocess64(crop, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """float64 restatement of one crop's resize + normalisation and the module docstring's bound e_x (times SAFETY), both [H, W, 3]."""
    H, W = size
    mean, std = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    p = crop.astype(np.float64) / 255.0
    h, w = p.shape[:2]
    cx, sx, fx = _taps64(W, w)
    cy, sy, fy = _taps64(H, h)
    x1, y1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    rows = p[:, sx] * (1.0 - fx)[None, :, None] + p[:, x1] * fx[None, :, None]
    v = rows[sy] * (1.0 - fy)[:, None, None] + rows[y1] * fy[:, None, None]
    dx = _local_max(np.abs(np.diff(p, axis=1)), sy, sx, (-1, 0, 1, 2), (-1, 0, 1))
    dy = _local_max(np.abs(np.diff(p, axis=0)), sy, sx, (-1, 0, 1), (-1, 0, 1, 2))
    x = (v - mean) / std
    e_t = U * (np.abs(cx) + 1.0)[None, :, None] * dx + U * (np.abs(cy) + 1.0)[:, None, None] * dy + 10 * U
    return x, SAFETY * (e_t / std + U * np.abs(x))


def conv_weights(seed=5):
    """Weights of the stem's first convolution with both signs: w [12, 2, 2, 3] as (co, kh, kw, c), bias [12]."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(12, 2, 2, 3)).astype(np.float32)
    b = rng.normal(size=12).astype(np.float32)
    assert (w > 0).any() and (w < 0).any() and (b > 0).any() and (b < 0).any()
    return w, b


def _patches(x):
    """[H, W, 3] -> [H / 2, W / 2, 12], the 2x2 stride-2 patches in (kh, kw, c) order."""
    H, W, _ = x.shape
    return x.reshape(H // 2, 2, W // 2, 2, 3).transpose(0, 2, 1, 3, 4).reshape(H // 2, W // 2, 12)


def front64(crop, w, b, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """float64 restatement of swin_crop_front_kernel on one crop and its bound: ([H / 2, W / 2, 12], the same shape)."""
    x, ex = preprocess64(crop, size, mean, std)                 # ex already carries SAFETY
    w64, b64 = np.asarray(w, np.float64).reshape(12, 12), np.asarray(b, np.float64)
    px, pe = _patches(x), _patches(ex)
    c1 = px @ w64.T + b64
    g12 = 12 * U / (1 - 12 * U)
    bound = pe @ np.abs(w64).T + SAFETY * g12 * (np.abs(px) @ np.abs(w64).T + np.abs(b64))
    return c1, bound
