"""Reference side of tests/test_gpu_postproc.py and tests/test_postproc_host.py (CPU only, no GPU import): float64 restatements of the
evaluation script's post-processing (csrc/postproc.hip, and diou_kernel of csrc/select.hip), the case tables and the bounds.

* camera de-biasing, reid/inference_utils.py:5-15: `debias64` (float64 throughout, the mean too, from the fp32 inputs), `debias_ref32` (the
  reference's own arithmetic: fp32 with a LAPACK inverse of the fp32 matrix - the yardstick of the tolerance), `cond` (the float64 condition
  number of X_c^T X_c + n_c la I) and `debias_two_steps64` (exactly two Newton-Schulz updates from I / ||A||_inf: what `iters = 2` computes).
* tracklet smoothing, reid/inference_utils.py:18-27: `smooth64`, with `keep` and an optional mask.
* descriptor, reid/image_reid_inference.py:112-123,252-253: `descriptor64` / `tta_descriptor64` with F.normalize's max(||x||, 1e-12).
* DIoU: oracle/matching.py:diou is float64 already and is used as it is.

BOUNDS.  u = 2^-24 (fp32 unit round-off).
* de-biasing: |got - debias64| <= 8 e_ref + 1e-6 per finite element, e_ref = max |debias_ref32 - debias64| of that camera.  An fp32 numpy
  emulation of the device chain (Gram matrix, ridge, Newton-Schulz with the device's stopping rule, projection, residual correction) stays
  within about 3 e_ref; the factor 8 leaves room for the device GEMM's summation order, 1e-6 for the final fp32 normalisation of unit rows.
* smoothing: u ((L + 1) mean_i |x_i[col]| + 4 |out|), L = valid rows of the tracklet: a sequential sum of L terms is off by at most
  (L - 1) u sum |x_i|, so the mean by (L - 1) u mean |x_i|; the division by L and the rounding of 1 - keep add u |avg| <= u mean |x_i| each:
  (L + 1) u mean |x_i| in all.  The two products and the final sum round once each, 4 u |out| with one to spare.  `keep` is the fp32
  value the entry receives (float(np.float32(keep))) and 1 - keep is formed from it in fp32, as the kernel forms it.
* descriptor: u (2 (d / 256 + 10) + 6), d = de + dl, absolute on elements of magnitude <= 1: a squared norm is 256 partial sums of d / 256
  products each, six shuffle steps and the 4-way sum over the waves (relative (d / 256 + 10) u), there are two norms in a row (the view's
  and the average's) and three divisions (by the view's norm, by 2 - exact -, by the final norm), each u, with slack for the square roots.
  Inputs keep magnitudes in [1e-3, 1e3] so that no fp32 square underflows or overflows: the oracle squares in float64, where neither happens.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
F = np.float32


# ---------------------------------------------------------------------------------------------- camera de-biasing
def _gram64(cur, la):
    cur = np.asarray(cur, np.float64)
    return cur.T @ cur + cur.shape[0] * float(la) * np.eye(cur.shape[1])


def cond(x_cam, la):
    """float64 2-norm condition number of X_c^T X_c + n_c la I (symmetric positive definite: the ratio of its extreme eigenvalues)"""
    w = np.linalg.eigvalsh(_gram64(x_cam, la))
    return float(w[-1] / w[0])


def _project_normalise64(cur, p):
    cen = cur - cur.mean(0)
    y = cen @ p.T
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / np.linalg.norm(y, axis=1, keepdims=True)


def debias_cam64(x_cam, la):
    """One camera's rows [n_c, d] (fp32 values) -> float64 [n_c, d]; a single row gives 0 / 0 = NaN as the reference does."""
    cur = np.asarray(x_cam, np.float64)
    return _project_normalise64(cur, np.linalg.inv(_gram64(cur, la)))


def _per_camera(x, cams, fn, dtype):
    x = np.asarray(x, np.float32)
    cams = np.asarray(cams)
    out = x.astype(dtype)
    for c in range(int(cams.max()) + 1):
        sel = cams == c
        if sel.any():                           # ids without rows are skipped (the reference's inverse of the zero matrix raises)
            out[sel] = fn(x[sel])
    return out


def debias64(x, cams, la=0.05):
    """diminish_camera_bias in float64 on the fp32 inputs -> float64 [n, d]"""
    return _per_camera(x, cams, lambda cur: debias_cam64(cur, la), np.float64)


def debias_cam_ref32(x_cam, la):
    cur = np.asarray(x_cam, F)
    n, d = cur.shape
    cen = cur - cur.mean(0, dtype=F)
    a = cur.T @ cur + F(n * la) * np.eye(d, dtype=F)
    p = np.linalg.inv(a)                        # float32 in, float32 LAPACK (sgesv) out
    assert p.dtype == F
    y = cen @ p.T
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / np.sqrt((y * y).sum(1, keepdims=True, dtype=F))


def debias_ref32(x, cams, la=0.05):
    """The same chain in the reference's arithmetic: fp32 with a LAPACK inverse of the fp32 matrix (CPU) -> float32 [n, d]"""
    return _per_camera(x, cams, lambda cur: debias_cam_ref32(cur, la), F)


def debias_two_steps64(x_cam, la):
    """What iters = 2 computes, in float64: X0 = I / ||A||_inf, two updates X <- X (2 I - A X), projection, normalisation"""
    cur = np.asarray(x_cam, np.float64)
    a = _gram64(cur, la)
    eye = np.eye(a.shape[0])
    x = eye / np.abs(a).sum(1).max()
    for _ in range(2):
        x = x @ (2.0 * eye - a @ x)
    return _project_normalise64(cur, x)


def debias_rows(seed, n, d, scale=1.0):
    """n rows: Gaussian plus a shared offset of 0.5 Gaussian (the camera's bias), normalised, times `scale`"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) + 0.5 * rng.standard_normal((1, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x * scale).astype(F)


KAPPA_REQUIRED = 150.0
KAPPA_STIFF = 3e4          # above it fp32 LAPACK itself is off by 1e-2
E_REF_REQUIRED = 2e-5
E_REF_STIFF = 3e-3
DEBIAS_D = (30, 130, 257)  # padded to 32, 132 and 260 columns on the device


def rows_of(d, tag):
    return {"2": 2, "5": 5, "d/2": d // 2, "d": d, "3d": 3 * d}[tag]


ROW_TAGS = ("2", "5", "d/2", "d", "3d")

# (d, rows tag, la, scale), thinned from DEBIAS_D x ROW_TAGS x {0.05, 5e-3, 5e-4} x {0.125, 1, 8}; kappa is computed, never assumed
# (tests/test_postproc_host.py holds every case to its class).
# MEASURED on one MI355X (profiles/postproc_gpu_tests.log): device error / e_ref per case, `before` = the Newton-Schulz inverse and the
# projection GEMM alone, `after` = with the two rounds of residual correction reid_cam_debias_dev now runs; the bound is 8 (+ 1e-6).
# Before, 2 required cases (9.1, 9.3) and 12 of the 15 stiff cases (up to 556) missed it; after, every case holds (worst 3.3).
#   class     case                       kappa   before    after
#   required  d30-n2-la0.05-s1             12.9     1.94     0.96
#   required  d30-n2-la0.005-s1             112     9.14     0.89
#   required  d30-n5-la0.005-s1            87.2     9.33     1.38
#   required  d30-nd_2-la0.005-s1          60.3     2.72     1.22
#   required  d30-nd-la0.05-s0.125         1.08     1.04     0.94
#   required  d30-n3d-la0.0005-s1          50.5     1.06     0.98
#   required  d30-n3d-la0.05-s8            40.6     1.06     0.99
#   required  d130-n2-la0.005-s1            104     5.19     2.68
#   required  d130-n5-la0.005-s0.125       2.07     4.44     3.33
#   required  d130-n5-la0.005-s1           70.9     6.30     1.89
#   required  d130-nd_2-la0.05-s1           5.9     1.31     0.85
#   required  d130-nd-la0.005-s1           46.6     1.31     1.11
#   required  d130-n3d-la0.05-s8           96.3     1.10     1.07
#   required  d257-n2-la0.0005-s0.125        21     3.09     2.25
#   required  d257-n2-la0.005-s1            129     5.77     1.26
#   required  d257-n5-la0.005-s1           69.6     2.81     1.12
#   required  d257-nd_2-la0.005-s1         44.1     1.81     1.28
#   required  d257-nd-la0.05-s1            5.38     1.51     1.28
#   required  d257-n3d-la0.005-s1            39     1.84     1.83
#   required  d257-n3d-la0.0005-s0.125     7.12     0.93     0.65
#   stiff     d30-n2-la0.005-s8        7.43e+03   371.59     0.95
#   stiff     d30-n5-la0.0005-s1            872    49.07     1.04
#   stiff     d30-nd_2-la0.05-s8            292    10.83     0.97
#   stiff     d30-nd-la0.0005-s8       2.49e+04   273.05     1.68
#   stiff     d130-n2-la0.0005-s1      1.33e+03   124.32     2.30
#   stiff     d130-n5-la0.005-s8       4.39e+03   431.80     2.16
#   stiff     d130-nd_2-la0.0005-s8    2.62e+04   192.45     2.08
#   stiff     d130-nd-la0.005-s8       2.15e+03     4.44     1.16
#   stiff     d130-nd-la0.0005-s8      2.49e+04    12.41     1.19
#   stiff     d130-n3d-la0.0005-s8          171     1.26     1.12
#   stiff     d257-n2-la0.005-s8       7.57e+03   556.25     3.00
#   stiff     d257-n5-la0.05-s8             483    15.33     1.40
#   stiff     d257-nd_2-la0.0005-s8    2.58e+04   190.41     1.78
#   stiff     d257-nd-la0.0005-s8      2.74e+04    36.30     1.13
#   stiff     d257-n3d-la0.005-s8           327     2.33     2.19
DEBIAS_REQUIRED = (          # kappa <= 150
    (30, "2", 0.05, 1.0), (30, "2", 5e-3, 1.0), (30, "5", 5e-3, 1.0), (30, "d/2", 5e-3, 1.0), (30, "d", 0.05, 0.125), (30, "3d", 5e-4, 1.0),
    (30, "3d", 0.05, 8.0),
    (130, "2", 5e-3, 1.0), (130, "5", 5e-3, 0.125), (130, "5", 5e-3, 1.0), (130, "d/2", 0.05, 1.0), (130, "d", 5e-3, 1.0), (130, "3d", 0.05, 8.0),
    (257, "2", 5e-4, 0.125), (257, "2", 5e-3, 1.0), (257, "5", 5e-3, 1.0), (257, "d/2", 5e-3, 1.0), (257, "d", 0.05, 1.0), (257, "3d", 5e-3, 1.0),
    (257, "3d", 5e-4, 0.125),
)
DEBIAS_STIFF = (             # 150 < kappa <= 3e4
    (30, "2", 5e-3, 8.0), (30, "5", 5e-4, 1.0), (30, "d/2", 0.05, 8.0), (30, "d", 5e-4, 8.0),
    (130, "2", 5e-4, 1.0), (130, "5", 5e-3, 8.0), (130, "d/2", 5e-4, 8.0), (130, "d", 5e-3, 8.0), (130, "d", 5e-4, 8.0), (130, "3d", 5e-4, 8.0),
    (257, "2", 5e-3, 8.0), (257, "5", 0.05, 8.0), (257, "d/2", 5e-4, 8.0), (257, "d", 5e-4, 8.0), (257, "3d", 5e-3, 8.0),
)


def debias_case(case):
    """-> (rows of the one camera, la); the seed is a function of the case alone"""
    d, tag, la, scale = case
    seed = d * 10000 + ROW_TAGS.index(tag) * 1000 + int(round(-100 * np.log10(la))) + int(scale * 8)
    return debias_rows(seed, rows_of(d, tag), d, scale), la


def case_id(case):
    return "d%d-n%s-la%g-s%g" % (case[0], case[1].replace("/", "_"), case[2], case[3])


ITERS2_CASE = (130, "5", 5e-3, 1.0)          # required class, kappa about 70: the case of the explicit iters = 2


def debias_bound(e_ref):
    return 8.0 * e_ref + 1e-6


# the structure case: five cameras with ids {0, 2, 3, 7, 9}, sizes in id order 3d, 2, d, 1, d / 2, rows interleaved
STRUCT_IDS = (0, 2, 3, 7, 9)


def struct_case(d, seed=77):
    sizes = (3 * d, 2, d, 1, d // 2)
    rng = np.random.default_rng(seed)
    x = np.concatenate([debias_rows(seed + 1 + i, m, d) for i, m in enumerate(sizes)], 0)
    cams = np.repeat(np.asarray(STRUCT_IDS, np.int32), sizes)
    perm = rng.permutation(len(cams))
    return np.ascontiguousarray(x[perm]), np.ascontiguousarray(cams[perm]), sizes


# ---------------------------------------------------------------------------------------------- tracklet smoothing
SMOOTH_D = (1, 255, 256, 257, 513)
SMOOTH_KEEP = (0.1, 0.5, 0.0, 1.0)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SMOOTH_LENGTHS = ((INT32_MAX, 1), (-5, 2), (INT32_MIN, 7), (3, 1000), (0, 1), (-1, 2))   # (sequence id, rows): unsorted, negative, extremes


def smooth_case(d, mask, seed=5):
    """x [1013, d], seqs (interleaved), valid: None, a mixed mask (it empties the tracklet with id -1 and thins the others) or all False"""
    rng = np.random.default_rng(seed + d)
    seqs = np.concatenate([np.full(m, s, np.int64) for s, m in SMOOTH_LENGTHS])
    seqs = seqs[rng.permutation(len(seqs))].astype(np.int32)
    x = (rng.standard_normal((len(seqs), d)) * 3.0 + 1.0).astype(F)
    if mask == "none":
        valid = None
    elif mask == "mixed":
        valid = rng.random(len(seqs)) < 0.7
        valid[seqs == -1] = False
        valid[seqs == INT32_MAX] = True
        valid[np.nonzero(seqs == INT32_MIN)[0][:2]] = True
    else:
        valid = np.zeros(len(seqs), bool)
    return x, seqs, valid


def smooth64(x, seqs, valid=None, keep=0.1):
    """-> (out float64 [n, d], bound float64 [n, d] - 0 where the row must come back bit for bit, L int [n] - valid rows of the row's
    tracklet, 0 for an invalid row)"""
    x = np.asarray(x, F)
    seqs = np.asarray(seqs)
    valid = np.ones(len(seqs), bool) if valid is None else np.asarray(valid).astype(bool)
    k = float(F(keep))
    k1 = float(F(1.0) - F(keep))                # the device forms 1 - keep in fp32
    out = x.astype(np.float64)
    bound = np.zeros(x.shape)
    count = np.zeros(len(seqs), np.int64)
    for j in np.unique(seqs):
        sel = (seqs == j) & valid
        if not sel.any():
            continue
        cur = x[sel].astype(np.float64)
        out[sel] = cur * k + cur.mean(0) * k1
        count[sel] = cur.shape[0]
        bound[sel] = U * ((cur.shape[0] + 1) * np.abs(cur).mean(0) + 4.0 * np.abs(out[sel]))
    return out, bound, count


# ---------------------------------------------------------------------------------------------- descriptor
DESC_DIMS = ((512, 751), (96, 1), (1, 1), (256, 256), (257, 300))
DESC_N = (1, 5)


def desc_bound(de, dl):
    d = de + dl
    return U * (2.0 * (d / 256.0 + 10.0) + 6.0)


def desc_inputs(seed, n, de, dl):
    """Two views (e1, l1, e2, l2) with magnitudes in [1e-3, 1e3]: every row has its own scale 10^U(-2.69, 2.69), its elements that scale times
    U(0.5, 2) with a random sign; the last row of l1 spreads log-uniformly over the whole range."""
    rng = np.random.default_rng(seed)

    def one(cols):
        s = 10.0 ** rng.uniform(-2.69, 2.69, (n, 1))
        return s * rng.uniform(0.5, 2.0, (n, cols)) * rng.choice([-1.0, 1.0], (n, cols))
    e1, l1, e2, l2 = one(de), one(dl), one(de), one(dl)
    l1[-1] = 10.0 ** rng.uniform(-2.99, 2.99, dl) * rng.choice([-1.0, 1.0], dl)
    out = [a.astype(F) for a in (e1, l1, e2, l2)]
    for a in out:
        assert (np.abs(a) >= 1e-3).all() and (np.abs(a) <= 1e3).all()
    return out


def _l2n64(x, eps=1e-12):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), eps)


def descriptor64(emb, logits):
    """cat of the two normalised halves; NOT renormalised"""
    return np.concatenate([_l2n64(emb), _l2n64(logits)], 1)


def tta_descriptor64(emb, logits, emb_flip, logits_flip):
    return _l2n64((descriptor64(emb, logits) + descriptor64(emb_flip, logits_flip)) / 2.0)


# x [rows][w] as the 256 x 128 entries mirror it (rows = images * 3 * 256, w = 128) and two tiny shapes.  The grid is capped at 8192 blocks of
# 256 threads: 8 images (786 432 elements) still get a thread per element, 22 images (2 162 688 > 8192 * 256) run the grid-stride loop.
FLIP_SHAPES = ((1, 1), (5, 7), (3 * 256 * 2, 128), (3 * 256 * 8, 128), (3 * 256 * 22, 128))


# ---------------------------------------------------------------------------------------------- DIoU
DIOU_SHAPES = ((1, 256), (1, 257), (3, 100), (40, 31))


def diou_boxes(t, m, seed=9):
    """tlwh boxes: random ones, then the special pairs - track i against detection i for i < 8 (when both exist), every special detection
    also against track 0, which is the box the specials are built around:
      0 identical, 1 disjoint, 2 contained, 3 edge-touching (intersection 0), 4 zero width, 5 all zero, 6 / 7 coordinates of 1e6"""
    rng = np.random.default_rng(seed + t * 1000 + m)

    def rand(k):
        return np.concatenate([rng.uniform(-50, 300, (k, 2)), rng.uniform(1, 120, (k, 2))], 1)
    tracks, dets = rand(t), rand(m)
    base = np.asarray([10.0, 20.0, 40.0, 80.0])
    tracks[0] = base
    special = np.asarray([
        base,                                   # identical: 1
        [500.0, 700.0, 30.0, 30.0],             # disjoint
        [20.0, 30.0, 10.0, 20.0],               # contained
        [50.0, 20.0, 25.0, 80.0],               # shares the edge x = 50: intersection 0
        [30.0, 40.0, 0.0, 50.0],                # zero width
        [0.0, 0.0, 0.0, 0.0],                   # all zero
        [1e6 + 3.0, -1e6 + 0.5, 37.0, 91.0],    # far away
        [1e6, 1e6, 1e6, 2e6],                   # huge
    ])
    k = min(len(special), m)
    dets[:k] = special[:k]
    for i in range(1, min(k, t)):
        tracks[i] = special[i]                  # pairs (i, i): identical boxes of every special kind, the all-zero PAIR among them
    return tracks, dets
