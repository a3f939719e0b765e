"""Numpy oracles of the evaluation chain's two links (csrc/eval_links.hip): the shifted mirrored view of the script's strong_inference
transform and the squared-domain bound of the attribute distance.  The yardstick of tests/test_eval_links_host.py and
tests/test_gpu_eval_links.py.

View (reid/data_transforms.py:130-191: Resize -> RandomHorizontalFlip(p=1) -> Pad(pad) -> RandomCrop((H, W)) -> ToTensor -> Normalize):
with (top, left) the crop's offsets into the padded image,

    sy = oy + top - pad;  sx = ox + left - pad;   y[c][oy][ox] = (0 <= sy < h and 0 <= sx < w) ? x[c][sy][w - 1 - sx] : fill[c]

which is crop(pad(mirror(x))); tests/test_eval_links_host.py checks it against Pillow's own transpose / expand / crop.

Distance (reid/losses/utils.py:21-35): v = sqrt(max(s_i + s_j - 2 a_i.a_j, 1e-12)) in fp32.  Where q is small against the norms the
square root magnifies the rounding of the dot product without limit, so the bound is set in the squared domain: with q the float64
value and b = (d + 3) 2^-24 (s_i + s_j + 2 |a_i|.|a_j|) - d roundings of the dot product's terms and chain, the two norms', the sum's
and the subtraction's, each at most 2^-24 of the magnitudes they round - a value v passes if

    sqrt(max(q - b, 1e-12)) - u <= v <= sqrt(max(q + b, 1e-12)) + u,     u one fp32 ulp of v (the square root's own rounding)."""
import numpy as np

SIZES = ((256, 128), (33, 47))
PADS = (10, 1, 0)


def shifts(pad):
    """The four corner shifts, the centre (the plain mirror) and (3, 17) clipped to [0, 2 pad] - without repeats."""
    out = []
    for tl in ((0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad), (pad, pad), (min(3, 2 * pad), min(17, 2 * pad))):
        if tl not in out:
            out.append(tl)
    return out


def shift_view(x, top, left, pad, fill, mirror=True, swap=False):
    """x [c][h][w] (any dtype) -> the view of the same shape; fill [c].  mirror=False / swap=True are the mutations: the source read
    unmirrored, top and left exchanged."""
    c, h, w = x.shape
    if swap:
        top, left = left, top
    oy, ox = np.arange(h)[:, None], np.arange(w)[None, :]
    sy, sx = oy + top - pad, ox + left - pad
    ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    syc, sxc = np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)
    src = x[:, syc, (w - 1 - sxc) if mirror else sxc]
    return np.where(ok[None], src, np.asarray(fill, x.dtype).reshape(c, 1, 1)).astype(x.dtype)


def shift_views(x, shift_tl, pad, fill, **kw):
    """x [n][c][h][w], shift_tl [n][2] -> [n][c][h][w]."""
    return np.stack([shift_view(x[i], int(shift_tl[i][0]), int(shift_tl[i][1]), pad, fill, **kw) for i in range(len(x))])


def dist_bounds(a, alpha=2.0):
    """a [n][d] -> (lo, hi) float64 [n][n] of the squared-domain bound WITHOUT the ulp term (inside() adds it)."""
    a64 = np.asarray(a, np.float64)
    d = a64.shape[1]
    s = (a64 * a64).sum(1)
    ss = s[:, None] + s[None, :]
    q = ss - alpha * (a64 @ a64.T)
    b = (d + 3) * 2.0 ** -24 * (ss + 2.0 * (np.abs(a64) @ np.abs(a64).T))
    return np.sqrt(np.maximum(q - b, 1e-12)), np.sqrt(np.maximum(q + b, 1e-12))


def ulp32(v):
    v = np.abs(np.asarray(v, np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def inside(v, lo, hi):
    """bool [n][n]: every fp32 value of v within [lo - u, hi + u], u one fp32 ulp of v; a NaN is outside."""
    v32 = np.asarray(v, np.float32)
    u = ulp32(v32)
    v64 = v32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (v64 >= lo - u) & (v64 <= hi + u)


def inside_sum(out, base, lo, hi):
    """The in-place add: out = fl(base + v) with v inside [lo, hi] up to its ulp - the bound of `inside` moved by base and widened by one
    ulp of the sum."""
    o32 = np.asarray(out, np.float32)
    b64 = np.asarray(base, np.float32).astype(np.float64)
    u = ulp32(o32) + np.maximum(ulp32(lo.astype(np.float32)), ulp32(hi.astype(np.float32)))
    o64 = o32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (o64 >= b64 + lo - u) & (o64 <= b64 + hi + u)


def euclid32(a, clamp=True, alpha=2.0):
    """A plain fp32 evaluation of the formula (numpy's own summation order) - the subject of the mutations."""
    a = np.asarray(a, np.float32)
    s = (a * a).sum(1, dtype=np.float32)
    q = (s[:, None] + s[None, :]) - np.float32(alpha) * (a @ a.T)
    if clamp:
        q = np.maximum(q, np.float32(1e-12))
    with np.errstate(invalid="ignore"):
        return np.sqrt(q).astype(np.float32)


def attribute_like_rows(n, d, seed):
    """Unit rows of d small integers (1 / 2, like the dataset's attributes) with many duplicates: n rows drawn from max(2, n // 3)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 3, (max(2, n // 3), d)).astype(np.float32)
    rows = base[rng.integers(0, len(base), n)]
    return (rows / np.sqrt((rows * rows).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
