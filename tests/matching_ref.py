"""Operands, float64 oracles and the shape tables of the exact-fp32 matching entries (reid_distmat*, reid_argmin_rows*, reid_knn*; the
two-pass selection kernels of csrc/select.hip and the fused ones of csrc/dist_select.hip), shared by tests/test_matching_host.py and
tests/test_gpu_matching.py.  Every input and reference is computed once per process and handed out read-only.

Families
  EXACT      integer features in -4 .. 4, d <= 2048: |x.y| <= 16 d and |x|^2 <= 16 d stay far below 2^24, so every partial sum of a dot
             product or a squared norm is an integer fp32 holds exactly IN ANY ORDER, and |x|^2 + |y|^2 - 2 x.y (<= 64 d) is exact too.
             DOT and L2SQR therefore have to equal the float64 oracle bit for bit; L2 is sqrtf of an exact integer (or of 1e-12);
             only the cosine forms round (allowance below).  Ties are real: y[n // 2] repeats y[3], x[0] equals y[3], integer data gives
             distinct rows at equal distance in abundance, and `identical=True` makes every gallery row the same vector.
  ROUNDED    N(0, 1) + offset (0 or 10: large norms, small distances - the cancellation case); some rows of y equal rows of x.
  NON-FINITE the rounded family with a NaN (sign bit clear) in a row of x, a NaN (sign bit set) in a row of y, an all-zero row in x and
             in y (0 / 0 under the cosine metrics) and, `infs=True` (DOT only), a +inf and a -inf entry in two rows of y.

Allowances (u = 2^-24), derived here and never tuned to what the kernels return
  exact family   DOT, L2SQR: 0.  L2: 1 ulp of float32(sqrt(max(v, 1e-12))) - IEEE sqrtf is within half an ulp, one ulp allows the device
                 sequence to round differently.  COS, COS_HALF: 8 u absolute - two square roots, a product, a division and a
                 subtraction round by at most u relative each, on quantities <= 1 up to rounding.
  rounded family |v - v64| <= B = (d + 4) u S.  Three sums of d terms (x.y, |x|^2, |y|^2) each carry at most (d - 1) u times their
                 absolute sum in any order (d u for an fma chain that starts from zero), plus the addition of the norms, the product
                 with 2 and the final fma: at most four more u on quantities bounded by S.
                   L2SQR  S = |x|^2 + |y|^2 + 2 sum_k |x_k y_k|          DOT  S = sum_k |x_k y_k|
                   L2     checked on its square against max(v64, 1e-12): the clamp is 1-Lipschitz, so the clamped value w is within B;
                          got = sqrtf(w) (1 + e), |e| <= u, so |got^2 - w| <= 3 u w <= 3 u (max(v64, 1e-12) + B):
                          BL2 = B + 3 u (max(v64, 1e-12) + B)
                   COS    the L2SQR bound divided by |x| |y|: (d + 4) u (|x|^2 + |y|^2 + 2 sum |x_k y_k|) / (|x| |y|) >= (d + 4) u (2 + 2 r)
                          with r = sum |x_k y_k| / (|x| |y|) >= |cos|, which covers d u (r + |cos|) from the dot product and the two
                          norms plus the roundings of the roots, the product, the division and 1 - q (each <= u on values <= 1 + r).
                   COS_HALF  half of it (the division by 2 is exact).
                 At d = 96 and 36 (d + 4) u is about 6e-6, far below an operand rounded to f16 or tf32 (2^-11): the bound notices a
                 wrong arithmetic, not only a wrong index.

The rule for NaN distances (include/reid_hip.h): a NaN of either sign bit is no candidate; reid_knn pads a row short of candidates
with (I = -1, D = +inf); reid_argmin_rows answers (idx = -1, val = NaN) for a row without any; +-inf are ordinary values; ties go to
the lowest column.  `select` below is that rule as np.lexsort((index, value)) over the non-NaN entries of a matrix.

Dispatch: `dist_form` and `select_form` restate launch_gemm_f32 / gemm_f32_dma_supported / launch_epi (csrc/gemm_f32.hip,
gemm_f32_dma.hip), pad_rows, select_fused_dev, knn_wide_eligible (csrc/api.hip, knn_wide.hip) and select_segments
(csrc/dist_select.hip); the tables name, row by row, the form a row reaches and why, and the host test asserts that the predicates
agree and that every form is reached.
"""
import functools

import numpy as np

METRIC_L2, METRIC_L2SQR, METRIC_COS_HALF, METRIC_COS, METRIC_DOT = range(5)
METRICS = {"L2": METRIC_L2, "L2SQR": METRIC_L2SQR, "COS_HALF": METRIC_COS_HALF, "COS": METRIC_COS, "DOT": METRIC_DOT}
U = 2.0 ** -24
COS_EXACT_ALLOW = 8 * U
NAN_POS = np.array([0x7fc00000], np.uint32).view(np.float32)[0]      # sign bit clear
NAN_NEG = np.array([0xffc00000], np.uint32).view(np.float32)[0]      # sign bit set: what x86 gives for inf - inf and 0 * inf


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------ dispatch predicates
DMA64, DMA128_K16, DMA128_K32, F32_64, F32_128 = "dma64", "dma128k16", "dma128k32", "f32_64", "f32_128"
DIST_FORMS = (DMA64, DMA128_K16, DMA128_K32, F32_64, F32_128)


def padded_k(d, x_off=0):
    """pad_rows: an operand whose d % 4 != 0, or whose pointer is off 16 bytes, is copied into zero-padded rows of ceil4(d) floats.  Both
    operands share d, so K = ceil4(d) either way; returns (K, copied)."""
    return (d + 3) // 4 * 4, d % 4 != 0 or (4 * x_off) % 16 != 0


def dist_form(m, n, d, x_off=0, f32_conv=1, bk16=1):
    """The kernel reid_distmat_dev launches.  launch_gemm_f32: the LDS-DMA kernel when f32_conv == 1 and gemm_f32_dma_supported (K % 32 == 0,
    16-byte rows and pointers - pad_rows has seen to those - and tiles below 2 GiB); launch_epi: the 64-wide tile when n <= 64 or
    ceil64(n) * 1.12 < ceil128(n), else the 128-wide one with K-tiles of 16 (f32_dist_bk16) or 32.  Otherwise gemm_f32_kernel
    (launch_bn): 64-wide for n <= 64, else 128-wide."""
    K = padded_k(d, x_off)[0]
    if f32_conv == 1 and K % 32 == 0 and 128 * K * 4 < 0x7fff0000:
        c64, c128 = (n + 63) // 64 * 64 * 1.12, (n + 127) // 128 * 128
        if n <= 64 or c64 < c128:
            return DMA64
        return DMA128_K16 if bk16 else DMA128_K32
    return F32_64 if n <= 64 else F32_128


def dist_tiles(m, n, form):
    """(full row tiles, ragged row tiles, column tiles, columns in the last column tile)"""
    bn = 64 if form in (DMA64, F32_64) else 128
    return m // 128, int(m % 128 != 0), (n + bn - 1) // bn, n - (n - 1) // bn * bn


def select_segments(m, n):
    """csrc/dist_select.hip select_segments"""
    nmt, nnt = (m + 127) // 128, (n + 127) // 128
    s = max(1, min(512 // nmt, nnt, 32))
    per = (nnt + s - 1) // s
    return (nnt + per - 1) // per


TWO_PASS_ARGMIN, TWO_PASS_TOPK, FUSED_ARGMIN, FUSED_SELECT, WIDE = "argmin_rows_kernel", "topk_rows_kernel", "fused_argmin", "fused_select", "knn_wide"
SELECT_FORMS = (TWO_PASS_ARGMIN, TWO_PASS_TOPK, FUSED_ARGMIN, FUSED_SELECT)


def select_form(m, n, d, k, entry="knn", two_pass=0, knn_wide=1, knn_wide_min=1 << 25):
    """The selection reid_knn_dev (entry "knn") / reid_argmin_rows_dev ("argmin", k = 1) runs.  knn_wide_eligible: k <= 24, n >= 4096,
    d >= 128, m n >= knn_wide_min; select_fused_dev: k <= 64, n >= 2048, m n >= 2^18 (rows are padded to K % 64 == 0 and 16-byte pointers,
    so dist_select_supported holds below 2 GiB tiles); otherwise the distance matrix and argmin_rows_kernel / topk_rows_kernel."""
    if not two_pass:
        if entry == "knn" and knn_wide and 1 <= k <= 24 and n >= 4096 and d >= 128 and m * n >= knn_wide_min:
            return WIDE
        if k <= 64 and n >= 2048 and m * n >= 1 << 18:
            return FUSED_ARGMIN if k == 1 else FUSED_SELECT
    return TWO_PASS_ARGMIN if entry == "argmin" else TWO_PASS_TOPK


# ------------------------------------------------------------------------------------------------ shape tables
# Distance matrix: (m, n, d, x_off, out_off, f32_conv, bk16, form).  x_off / out_off: floats by which x / the output is moved off its
# allocation.  The last field is what the row is meant to reach; the host test holds it against dist_form.
# Rows m: 1 = one ragged tile, 128 = one full tile (the buffer-store branch of dist_epilogue), 129 = a full tile next to a ragged one.
# Columns n: 1 and 64 = one 64-wide tile (n <= 64); 65 = 128-wide by the cost model (128 * 1.12 > 128); 129 = 64-wide (192 * 1.12 = 215 <
# 256) with three column tiles, the last of one column; 193 = 128-wide (256 * 1.12 > 256) with two tiles.
def _rows():
    t = []
    for d in (32, 96):     # d = 32: one K-tile of 32 (two of 16); d = 96: three K-tiles of 32, the odd tail of the two-stage loop
        for m in (1, 128, 129):
            t += [
                (m, 1, d, 0, 0, 1, 1, DMA64),            # one column: every lane but one is past the edge
                (m, 64, d, 0, 0, 1, 1, DMA64),           # the widest gallery of the n <= 64 rule
                (m, 65, d, 0, 0, 1, 1, DMA128_K16),      # the narrowest gallery the cost model gives the 128-wide tile, K-tiles of 16
                (m, 65, d, 0, 0, 1, 0, DMA128_K32),      # ... and K-tiles of 32
                (m, 129, d, 0, 0, 1, 1, DMA64),          # three 64-wide column tiles, the last of one column
                (m, 193, d, 0, 0, 1, 1, DMA128_K16),     # two 128-wide column tiles, the second of 65 columns
                (m, 193, d, 0, 0, 1, 0, DMA128_K32),
            ]
    return t


DIST_TABLE = tuple(_rows()) + (
    (129, 193, 96, 0, 3, 1, 1, DMA128_K16),   # the output three floats off its allocation: buffer stores and the guard in front of it
    (129, 129, 96, 0, 1, 1, 1, DMA64),        # the same for the 64-wide tile
    (129, 64, 4, 0, 0, 1, 1, F32_64),         # K % 32 != 0: gemm_f32_kernel, one K-tile of which four columns are real; 64-wide
    (129, 65, 4, 0, 0, 1, 1, F32_128),        # ... 128-wide (n > 64)
    (129, 64, 36, 0, 0, 1, 1, F32_64),        # a full K-tile and a ragged one
    (129, 65, 36, 0, 0, 1, 1, F32_128),
    (129, 1, 36, 0, 0, 1, 1, F32_64),         # its 64-wide tile with a column edge
    (1, 65, 36, 0, 0, 1, 1, F32_128),         # a ragged-only row tile of gemm_f32_kernel
    (129, 64, 96, 0, 0, 0, 1, F32_64),        # f32_conv = 0: gemm_f32_kernel on a shape the LDS-DMA kernel would take
    (129, 193, 96, 0, 0, 0, 1, F32_128),      # ... two 128-wide column tiles
    (129, 65, 1, 0, 0, 1, 1, F32_128),        # d % 4 != 0: the pad_rows copy (K = 4, three zero columns)
    (3, 64, 33, 0, 0, 1, 1, F32_64),          # the copy with K = 36
    (129, 65, 33, 0, 0, 1, 1, F32_128),
    (129, 65, 32, 1, 0, 1, 1, DMA128_K16),    # x four bytes off a 16-byte boundary: the copy although d % 4 == 0, then the LDS-DMA kernel
    (129, 65, 2048, 0, 0, 1, 1, DMA128_K16),  # a long K for the accumulator: 128 K-tiles of 16
    (129, 65, 2048, 0, 0, 1, 0, DMA128_K32),  # ... 64 of 32
    (129, 64, 2048, 0, 0, 0, 1, F32_64),      # ... and gemm_f32_kernel's loop
)
# the rounded family runs at d = 96 and 36, where (d + 4) u ~ 6e-6, on the rows with a full and a ragged tile
ROUNDED_TABLE = tuple(r for r in DIST_TABLE if r[2] in (96, 36) and r[0] == 129)

# Selection: (m, n, d, k, identical gallery, form of reid_knn_dev).  d = 64 keeps the wide path (d >= 128) out.
SELECT_TABLE = (
    (3, 300, 32, 1, False, TWO_PASS_TOPK),      # n < 2048: the matrix, then topk_rows_kernel with k = 1 (argmin_rows_kernel for the arg-min entry)
    (3, 300, 32, 5, False, TWO_PASS_TOPK),      # ... two strides of the 256 threads over a row
    (2, 5, 32, 8, False, TWO_PASS_TOPK),        # k > n: three columns of padding
    (128, 2049, 64, 1, False, FUSED_ARGMIN),    # m n = 2^18 + 128: 17 column tiles, the last of one column, one row tile, S = 17
    (128, 2049, 64, 7, False, FUSED_SELECT),
    (128, 2049, 64, 64, False, FUSED_SELECT),   # k = SEL_KMAX: a list is compacted to as many keys as trigger the compaction
    (129, 2049, 64, 7, False, FUSED_SELECT),    # two row tiles, the second of one row
    (70, 4200, 64, 1, False, FUSED_ARGMIN),     # 33 column tiles: 17 segments of two tiles (the last of one)
    (70, 4200, 64, 20, False, FUSED_SELECT),
    (128, 2049, 64, 65, False, TWO_PASS_TOPK),  # k > 64: just outside the fused range
    (127, 2049, 64, 7, False, TWO_PASS_TOPK),   # m n = 2^18 - 1921 < 2^18: just outside
    (128, 2049, 64, 1, True, FUSED_ARGMIN),     # every gallery row the same vector: every element ties with the threshold
    (128, 2049, 64, 20, True, FUSED_SELECT),    # ... the answer is columns 0 .. 19
)
NONFINITE_SHAPES = ((3, 300, 32), (128, 2049, 64))     # two-pass, fused


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def exact_operands(m, n, d, identical=False, seed=5):
    """Integers in -4 .. 4.  y[n // 2] = y[3] and x[0] = y[3] (n >= 8): a zero distance, and a tie between two columns that the lower one
    wins; x[m - 1] = y[n - 1]: a zero in the last row and column.  identical: every row of y is y[0]."""
    rng = np.random.default_rng(seed + 1000003 * m + 1009 * n + d)
    x = rng.integers(-4, 5, (m, d)).astype(np.float32)
    y = rng.integers(-4, 5, (n, d)).astype(np.float32)
    if identical:
        y[:] = y[0]
    elif n >= 8:
        y[n // 2] = y[3]
        x[0] = y[3]
        x[m - 1] = y[n - 1]
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def rounded_operands(m, n, d, offset=0.0, seed=7):
    """N(0, 1) + offset; y[j] = x[j % m] for every seventh j: distances that cancel to (about) zero."""
    rng = np.random.default_rng(seed + 1000003 * m + 1009 * n + d)
    x = (rng.normal(size=(m, d)) + offset).astype(np.float32)
    y = (rng.normal(size=(n, d)) + offset).astype(np.float32)
    for j in range(0, n, 7):
        y[j] = x[j % m]
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def nonfinite_operands(m, n, d, infs=False, seed=9):
    """The rounded family with: x[1] carrying a NaN (sign clear), y[2] a NaN (sign set), x[m - 1] and y[n - 1] all zero, and with `infs`
    y[4] one +inf and y[n - 2] one -inf entry (DOT: x rows have no zeros but the all-zero row, whose products with them are NaN)."""
    x, y = (a.copy() for a in rounded_operands(m, n, d, 0.0, seed))
    x[1, d // 2] = NAN_POS
    y[2, d - 1] = NAN_NEG
    x[m - 1] = 0.0
    y[n - 1] = 0.0
    if infs:
        y[4, 1] = np.inf
        y[n - 2, 0] = -np.inf
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def nan_gallery_operands():
    """(2, 5, 32): three of the five gallery rows carry a NaN (both sign bits), and query 1 carries one: fewer candidates than k = 4."""
    x, y = (a.copy() for a in rounded_operands(2, 5, 32, 0.0, 13))
    y[0, 3], y[2, 31], y[3, 0] = NAN_NEG, NAN_POS, NAN_NEG
    x[1, 7] = NAN_NEG
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def one_thread_operands():
    """topk_rows_kernel keeps four keys per thread; gallery rows 7, 263, 519, ... (what thread 7 of the 256 visits) are the twelve nearest
    neighbours of every query, so that thread's list runs dry and the row takes the exact fallback.  Exact family: the near rows have
    i + 1 ones (|y|^2 <= 12), the queries one +-1, every other row entries of magnitude 2 .. 4 (distance >= (sqrt(128) - 1)^2 > 100,
    against (1 + sqrt(12))^2 < 20).  (6, 3000, 32): m n < 2^18, so reid_knn takes the two-pass form."""
    rng = np.random.default_rng(21)
    xb = (rng.integers(2, 5, (3000, 32)) * rng.choice([-1, 1], (3000, 32))).astype(np.float32)
    near = np.arange(7, 3000, 256)
    xb[near] = 0.0
    for i, r in enumerate(near):
        xb[r, :i + 1] = 1.0
    xq = np.zeros((6, 32), np.float32)
    xq[np.arange(6), rng.integers(0, 32, 6)] = rng.choice([-1.0, 1.0], 6)
    return _ro(xq, xb, near)


# ------------------------------------------------------------------------------------------------ oracles
def oracle(x, y, metric):
    """float64, the reference's formulas (reid/losses/utils.py:12-35; DOT = x y^T; COS = 2 COS_HALF), NaN and inf propagated as numpy does."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        dot = x64 @ y64.T
        if metric == METRIC_DOT:
            return dot
        xx, yy = (x64 * x64).sum(1)[:, None], (y64 * y64).sum(1)[None, :]
        if metric in (METRIC_L2, METRIC_L2SQR):
            v = xx + yy - 2.0 * dot
            if metric == METRIC_L2SQR:
                return v
            return np.sqrt(np.where(v < 1e-12, 1e-12, v))          # clamp(min=1e-12) keeps NaN
        c = 1.0 - dot / (np.sqrt(xx) * np.sqrt(yy))
        return c if metric == METRIC_COS else c / 2.0


def bound(x, y, metric):
    """The rounded family's allowance (module docstring), per element; for L2 on the SQUARE against max(v64, 1e-12)."""
    ax, ay = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
    d = ax.shape[1]
    sabs = ax @ ay.T
    if metric == METRIC_DOT:
        return (d + 4) * U * sabs
    xx, yy = (ax * ax).sum(1)[:, None], (ay * ay).sum(1)[None, :]
    b = (d + 4) * U * (xx + yy + 2.0 * sabs)
    if metric == METRIC_L2SQR:
        return b
    if metric == METRIC_L2:
        return b + 3 * U * (np.maximum(oracle(x, y, METRIC_L2SQR), 1e-12) + b)
    b = b / (np.sqrt(xx) * np.sqrt(yy))
    return b if metric == METRIC_COS else b / 2.0


def rounded_share(got, x, y, metric):
    """max |got - float64| / bound over the matrix (L2: on the square)."""
    got = np.asarray(got, np.float64)
    if metric == METRIC_L2:
        err = np.abs(got * got - np.maximum(oracle(x, y, METRIC_L2SQR), 1e-12))
    else:
        err = np.abs(got - oracle(x, y, metric))
    return float((err / bound(x, y, metric)).max())


def ulp_distance(a, b):
    """|a - b| in units of float32's last place, for non-negative floats of the same sign"""
    return np.abs(np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64))


def exact_mismatch(got, x, y, metric):
    """Exact family: the number of elements outside the allowance of the module docstring (0 for DOT / L2SQR: bit for bit)."""
    want = oracle(x, y, metric)
    got = np.asarray(got, np.float32)
    nan = np.isnan(want)                                           # d = 1: a zero against a zero under the cosine metrics
    bad = np.isnan(got) != nan
    if metric in (METRIC_DOT, METRIC_L2SQR):
        return int((bad | (got.view(np.uint32) != want.astype(np.float32).view(np.uint32))).sum())
    if metric == METRIC_L2:
        return int((bad | (ulp_distance(got, want.astype(np.float32)) > 1)).sum())
    with np.errstate(invalid="ignore"):
        return int((bad | (~nan & ~(np.abs(got.astype(np.float64) - want) <= COS_EXACT_ALLOW))).sum())


def select(mat, k):
    """The rule: per row the k smallest non-NaN entries by (value, column), padded with (+inf, -1).  Returns (D like mat, I int32)."""
    mat = np.asarray(mat)
    m, n = mat.shape
    D = np.full((m, k), np.inf, mat.dtype)
    I = np.full((m, k), -1, np.int32)
    cols = np.arange(n)
    for i in range(m):
        keep = ~np.isnan(mat[i])
        order = cols[keep][np.lexsort((cols[keep], mat[i][keep]))][:k]
        D[i, :len(order)] = mat[i][order]
        I[i, :len(order)] = order
    return D, I


def argmin_rule(mat):
    """(idx, val) of reid_argmin_rows under the rule: a row without a non-NaN entry answers (-1, NaN)."""
    D, I = select(mat, 1)
    val = np.where(I[:, 0] < 0, np.nan, D[:, 0]).astype(np.asarray(mat).dtype)
    return I[:, 0], val


def decided_rows(x, y, metric):
    """Rows whose float64 winner leads the runner-up by more than twice the cosine allowance (n >= 2)."""
    D, _ = select(oracle(x, y, metric), 2)
    return (D[:, 1] - D[:, 0]) > 2 * COS_EXACT_ALLOW


def enough_decided(decided):
    """At least nine rows in ten.  Row 0 is undecided by construction (x[0] = y[3] = y[n // 2]: an exact tie), which a table row of two or
    three queries cannot absorb: there every other row has to be decided."""
    return decided.sum() >= min(0.9 * len(decided), len(decided) - 1)


# ------------------------------------------------------------------------------------------------ DIoU cases
@functools.lru_cache(maxsize=None)
def diou_cases():
    """name -> (tracks [t, 4], dets [m, 4]) tlwh float64: t m of 255, 256, 257 (the last block's edge), negative and huge coordinates,
    touching, nested, zero-width and identical zero-size boxes (0 / 0 in both terms: NaN in numpy and on the device)."""
    rng = np.random.default_rng(3)

    def boxes(n, lo=0.0, scale=100.0):
        return np.concatenate([lo + scale * rng.random((n, 2)), 1.0 + 0.5 * scale * rng.random((n, 2))], 1)
    special = np.array([[0, 0, 10, 10], [10, 0, 10, 10], [10, 10, 5, 5], [2, 2, 3, 3], [0, 0, 0, 10], [5, 5, 0, 0], [5, 5, 0, 0],
                        [-20, -30, 10, 10], [-5, -5, 10, 10], [0, 5, 10, 0]], np.float64)
    return {
        "t15_m17_255": _ro(boxes(15), boxes(17)),
        "t16_m16_256": _ro(boxes(16), boxes(16)),
        "t1_m257": _ro(boxes(1), boxes(257)),
        "negative": _ro(boxes(7, -300.0), boxes(9, -280.0)),
        "near_1e8": _ro(boxes(5, 1e8, 50.0), boxes(6, 1e8, 50.0)),
        "touching_nested_zero": _ro(special.copy(), special.copy()),
    }
