"""numpy restatement of the fp32-class distance matrix (csrc/distmat_x3.hip, reid_distmat_x3*), its float64 oracle with the derived error
bounds, and the inputs its tests share (every input and reference is computed once per process and handed out read-only).

Arithmetic: xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11), yh = f16_rn(y), yq = f16(yh 2^11), yl' = f16_rn((y - yh) 2^11),
all kept with f16's subnormals; dot[i][j] = 2^-11 sum_k (xh yq + xl' yh + xh yl').  `restate` holds the parts as np.float16 and sums in
float64: the kernel's value without its fp32 accumulation error.  On the EXACT family every term is a multiple of 0.25 and the sum of
magnitudes stays below 2^24 quarters, so fp32 accumulation is exact in any order and the kernel has to return float32(restate) bit for
bit.  The SMALL family (|x| ~ 2^-15) puts xh in and xl' at the edge of f16's subnormal range.

Error bounds (derived here, not tuned; u = 2^-24, u16 = 2^-11).  Per element of an operand row, with v = vh + vl:
  |vl| <= u16 |v| + 2^-25 =: L          (one f16 rounding; 2^-25 = half a subnormal step, the absolute term below f16's normal range)
  |vl' 2^-11 - vl| <= u16 L + 2^-36 =: D  (the rounding of vl 2^11 to f16; 2^-36 = 2^-25 2^-11)
  |vh| <= |v| + L =: H;  yq = yh 2^11 is exact inside the domain.
The kernel forms xh yh + xl~ yh + xh yl~ (v~ = vl' 2^-11) for (xh + xl)(yh + yl): the error per k is (xl~ - xl) yh + xh (yl~ - yl) - xl yl,
  E_split = Dx Hy^T + Hx Dy^T + Lx Ly^T             (matrix products of the elementwise bounds: ~ 3 2^-22 sum_k |x_k||y_k|)
and the 3 ld terms are summed in fp32 in an order the matrix unit does not document.  Its adder is not documented to round to nearest
either, so a rounding there is taken as |delta| < 2^-23 (a truncating adder), and n additions of terms of total magnitude Mag cost at
most gamma(n) Mag, gamma(n) = n 2^-23 / (1 - n 2^-23):
  Mag = Hx Hy^T + (Lx + Dx) Hy^T + Hx (Ly + Dy)^T,   E_dot = E_split + gamma(3 ld) Mag + 2^-149    (the last: acc 2^-11 in fp32)
The exact entry (fp32 MFMA: a rounded product and an addition per k) gets E_exact = gamma(2 ld) sum_k |x_k||y_k| + 2^-149.
Squared norms (row_sqnorm_kernel: a lane adds ceil(ld / 64) squares - product and sum, or one fma -, then six butterfly additions of
non-negative numbers, IEEE round-to-nearest): rs^ = rs (1 + t), |t| <= g = gamma_u(ceil(ld / 64) + 7), gamma_u(n) = n u / (1 - n u).
Through the formulas of gemm_f32_dma.hip (sqrtf and the division are correctly rounded in HIP's default build; every VALU result
carries one u):
  L2SQR  v = fma(-2, dot^, fl(rs^ + cq^)):  Es = g (rs + cq) (1 + u) + u (rs + cq),  B2 = (Es + 2 E_dot)(1 + u) + u |d2|
  L2     got = sqrtf(max(v, 1e-12f)); asserted on got^2:  |max(v, 1e-12) - d2| <= 2 B2 + 2e-12 =: W (v >= -B2 because d2 >= 0), and
         got^2 = max(..)(1 + u)^2:  BL2 = W + 3u (d2 + W).  Where d2 < BL2 the assertion is got <= sqrt(max(d2 + BL2, 1e-12)) (1 + 2^-22).
  COS    p = fl(fl(sqrt rs^) fl(sqrt cq^)) = |x||y| (1 + eta), |eta| <= ETA = (1 + g)(1 + u)^3 - 1;  q = fl(dot^ / p), c = dot / (|x||y|):
         Bq = (|c| ETA + E_dot / (|x||y|)) / (1 - ETA) (1 + u) + u |c|;  v = fl(1 - q):  BCOS = Bq + u (|1 - c| + Bq)
  COS_HALF  half of BCOS (the division by 2 is exact);  DOT  E_dot.
"""
import functools

import numpy as np

METRIC_L2, METRIC_L2SQR, METRIC_COS_HALF, METRIC_COS, METRIC_DOT = range(5)
METRICS = {"L2": METRIC_L2, "L2SQR": METRIC_L2SQR, "COS_HALF": METRIC_COS_HALF, "COS": METRIC_COS, "DOT": METRIC_DOT}
# (m, n, d): the smallest shapes at which each path can go wrong
SHAPES = (
    (1, 1, 1),            # the smallest problem
    (5, 3, 32),           # one ragged tile, n % 4 != 0
    (127, 129, 96),       # tile edges on both sides, odd n
    (130, 70, 100),       # d % 32 != 0 with 16-byte-aligned rows
    (3, 300, 33),         # d % 4 != 0, so the padded copy
    (200, 260, 160),      # several tiles both ways
    (40, 64, 64),         # the widest gallery of the 128 x 64 tile form (n % 4 == 0: 16-byte stores)
    (40, 68, 64),         # the narrowest n % 4 == 0 gallery of the 128 x 128 form
)
FORM_128x64, FORM_128x128 = 1, 2
F16_MIN_NORMAL = 2.0 ** -14
U, U16 = 2.0 ** -24, 2.0 ** -11
U_ACC = 2.0 ** -23


def form_of(n):
    """distmat_x3.h: the tile form is a rule of n alone."""
    return FORM_128x64 if n <= 64 else FORM_128x128


def ld_of(d):
    return (d + 31) // 32 * 32


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def exact_operands(m, n, d, seed=11):
    """x = (+-1 + l 2^-13) kept with probability 0.25 (0 otherwise; d = 1 keeps its one entry), y the same with every entry kept,
    l in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        return (rng.choice([-1.0, 1.0], shape) + rng.integers(-1, 2, shape) * 2.0 ** -13).astype(np.float32)
    x = (draw((m, d)) * ((rng.random((m, d)) < 0.25) | (d == 1))).astype(np.float32)
    return _ro(x, draw((n, d)))


@functools.lru_cache(maxsize=None)
def random_operands(m, n, d, seed=21, unit=False):
    """Standard normal rows (unit: scaled to length 1 in float64, then rounded).  The cancellation case: rows 0, 2, 4.. of y (as far as x
    has them) are rows of x, rows 1, 3, 5.. are rows of x with 2^-10 relative noise per element."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(m, d))
    y = rng.normal(size=(n, d))
    k = min(m, n)
    y[:k] = x[:k]
    y[1:k:2] *= 1.0 + 2.0 ** -10 * rng.uniform(-1, 1, size=y[1:k:2].shape)
    if unit:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        y /= np.linalg.norm(y, axis=1, keepdims=True)
    x = x.astype(np.float32)
    y = y.astype(np.float32)
    y[0:k:2] = x[0:k:2]
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def small_operands(m, n, d, seed=12):
    rng = np.random.default_rng(seed)
    return _ro((rng.normal(size=(m, d)) * 2.0 ** -15).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rank_operands(seed=7):
    """64 queries and 200 gallery rows of width 512, unit length (the seed: one at which no row's float64 top-2 gap lies inside the bounds,
    tests/test_distmat_x3_host.py::test_rank_input_has_clear_winners)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(64, 512))
    y = rng.normal(size=(200, 512))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return _ro(x.astype(np.float32), y.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the restatement
def _flush(part):
    return np.where(np.abs(part) < F16_MIN_NORMAL, 0.0, part)


def split(v, flush_hi=False, flush_lo=False):
    """fp32 -> (hi, lo') as float64 arrays holding f16 values; flush_*: that part without f16's subnormals (the mutation)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    return (_flush(hi) if flush_hi else hi), (_flush(lo) if flush_lo else lo)


def restate(x, y, drop=None, swap_qh=False, flush_hi=False, flush_lo=False):
    """(value, magnitude): 2^-11 (xh.yq + xl'.yh + xh.yl') in float64 on every element [m, n], and the sum of the terms' magnitudes on
    the accumulator's scale (before the 2^-11).  Mutations: drop "lh" leaves xl'.yh out, "hl" xh.yl'; swap_qh exchanges yq and yh;
    flush_*: the parts of x without f16's subnormals."""
    xh, xl = split(x, flush_hi, flush_lo)
    yh, yl = split(y)
    yq = (yh.astype(np.float32) * np.float32(2048.0)).astype(np.float16).astype(np.float64)
    assert np.isfinite(yq).all()
    if swap_qh:
        yq, yh = yh, yq
    acc = xh @ yq.T
    mag = np.abs(xh) @ np.abs(yq).T
    if drop != "lh":
        acc = acc + xl @ yh.T
        mag = mag + np.abs(xl) @ np.abs(yh).T
    if drop != "hl":
        acc = acc + xh @ yl.T
        mag = mag + np.abs(xh) @ np.abs(yl).T
    return acc * 2.0 ** -11, mag


# ------------------------------------------------------------------------------------------------ float64 oracle and bounds
def gamma(n, u):
    return n * u / (1.0 - n * u)


def dot_bounds(x, y):
    """(dot, A, E_dot, E_exact) in float64: the dot products, sum_k |x_k||y_k|, and the bounds of the module docstring for the fp32-class
    and for the exact entry."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ld = ld_of(x64.shape[1])
    ax, ay = np.abs(x64), np.abs(y64)
    lx, ly = U16 * ax + 2.0 ** -25, U16 * ay + 2.0 ** -25
    dx, dy = U16 * lx + 2.0 ** -36, U16 * ly + 2.0 ** -36
    hx, hy = ax + lx, ay + ly
    e_split = dx @ hy.T + hx @ dy.T + lx @ ly.T
    mag = hx @ hy.T + (lx + dx) @ hy.T + hx @ (ly + dy).T
    a = ax @ ay.T
    return x64 @ y64.T, a, e_split + gamma(3 * ld, U_ACC) * mag + 2.0 ** -149, gamma(2 * ld, U_ACC) * a + 2.0 ** -149


def oracle(x, y, metric, e_dot=None):
    """(want, bound) in float64 for one metric; for L2 `want` is the SQUARED distance and the bound is on got^2 (module docstring).
    e_dot: the dot product's bound (default: the fp32-class entry's)."""
    dot, a, e3, _ = dot_bounds(x, y)
    e = e3 if e_dot is None else e_dot
    if metric == METRIC_DOT:
        return dot, e
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rs, cq = (x64 * x64).sum(1)[:, None], (y64 * y64).sum(1)[None, :]
    g = gamma(-(-ld_of(x64.shape[1]) // 64) + 7, U)
    if metric in (METRIC_L2, METRIC_L2SQR):
        d2 = ((x64[:, None, :] - y64[None, :, :]) ** 2).sum(2) if x64.shape[0] * y64.shape[0] * x64.shape[1] <= 1 << 24 else rs + cq - 2 * dot
        es = g * (rs + cq) * (1 + U) + U * (rs + cq)
        b2 = (es + 2 * e) * (1 + U) + U * np.abs(d2)
        if metric == METRIC_L2SQR:
            return d2, b2
        w = 2 * b2 + 2e-12
        return d2, w + 3 * U * (d2 + w)
    nn = np.sqrt(rs) * np.sqrt(cq)
    c = dot / nn
    eta = (1 + g) * (1 + U) ** 3 - 1
    bq = (np.abs(c) * eta + e / nn) / (1 - eta) * (1 + U) + U * np.abs(c)
    bcos = bq + U * (np.abs(1 - c) + bq)
    return (1 - c, bcos) if metric == METRIC_COS else ((1 - c) / 2, bcos / 2)


def check(got, x, y, metric, e_dot=None):
    """Largest error / bound of `got` (fp32 [m, n]) against the oracle, by the issue's rule for L2: got^2 against the float64 squared
    distance, and where that lies below the bound got <= sqrt(max(d2 + bound, 1e-12)) (1 + 2^-22).  Returns (share, ok)."""
    want, b = oracle(x, y, metric, e_dot)
    g = np.asarray(got, np.float64)
    if metric != METRIC_L2:
        share = np.abs(g - want) / b
        return float(share.max()), bool((share <= 1.0).all())
    tiny = want < b
    share = np.where(tiny, 0.0, np.abs(g * g - want) / b)
    cap = np.sqrt(np.maximum(want + b, 1e-12)) * (1 + 2.0 ** -22)
    ok = (share <= 1.0).all() and (g[tiny] <= cap[tiny]).all() and (g >= 0).all()
    return float(share.max()), bool(ok)


def rank_rows(x, y, metric):
    """(best, clear): the float64 arg-min of every row, and the rows whose float64 top-2 gap exceeds the sum of both entries' bounds - taken
    at the row's largest bound and on both sides of the gap, so that neither entry can prefer another column on such a row."""
    want, b3 = oracle(x, y, metric)
    _, b0 = oracle(x, y, metric, dot_bounds(x, y)[3])
    s = np.sort(want, axis=1)
    return want.argmin(1), (s[:, 1] - s[:, 0]) > 2 * (b3 + b0).max(1)
