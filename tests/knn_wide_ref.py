"""numpy restatement, operand families and shape table of the large k-NN path (csrc/knn_wide.hip; reid_knn* for k <= 24, nb >= 4096,
d >= 128, nq nb >= knn_wide_min), shared by tests/test_knn_wide_host.py and tests/test_gpu_knn_wide.py.  The float64 oracle, the rule's
`select`, the exact / rounded / non-finite operands and the NaN constants are those of tests/matching_ref.py.

The path, per call (ld = ceil64(d), nbpad = ceil256(nb)):
  scales   sx = 2^-e with 2^e > sqrt(max |x|^2) >= 2^(e - 1) (frexpf; 1 for an all-zero or non-finite maximum; e within +-100), sy likewise:
           every scaled component lies in [-1, 1], a maximum that is exactly 2^p gives 2^-(p + 1);
  matrix   sx sy (|y|^2 - 2 x.y), the dot product of the scaled operands as three f16 products per multiply with fp32 accumulation
           (tests/distmat_x3_ref.py's split / restate);
  rowsel   threshold = the largest of the 32 minima of the groups `column mod 32`; the columns at or below it are the survivors; more
           than CAP = 1024 of them flag the row; else the KK = 32 smallest by (key, column) are the candidates;
  refine   the candidates' exact fp32 distances, the k smallest by (value, column);
  proof    the k-th exact value, less |x|^2 and times sx sy, plus err stays strictly below the 32nd candidate's matrix value minus err -
           else the row is flagged;
  fallback a flagged row is answered from all nb exact distances, NaN no candidate;
  whole    a squared norm that is NaN or +inf in fp32 (scale_prep_kernel reads them all anyway) flags every row of the call, and the
           query pack raises no range fault: reid_knn's rule for NaN distances holds whichever path a shape takes.

err = err_scale (|x|^2 + max |y|^2) sx sy + err_abs, per row, in the matrix's units:
  err_scale = (6 ld / 16 + 16) 2^-24, restated from knn_wide.hip: the three-product split loses 3 x 2^-22 |x| |y| (22-bit operands, the
           xl.yl term), the fp32 accumulator rounds once or twice per MFMA over 3 ld / 16 of them; times two for the factor -2, with
           |x| |y| <= (|x|^2 + |y|^2) / 2; the + 16 holds the 12 of the split, the bias product and the epilogue's fma;
  err_abs   = ld 2^-32: f16 has no bits below 2^-24, so a scaled component v splits with ABSOLUTE errors besides the relative ones:
           |v - vh| <= 2^-11 |v| + 2^-25, |v - vh - vl| <= 2^-11 |v - vh| + 2^-36.  Per multiply of scaled |a|, |b| <= 1 the terms the
           relative bound does not hold are 2^-25 2^-11 (a + b) + 2^-50 (xl.yl) and 2 x 2^-36 b + 2 x 2^-36 a (the lost low bits against
           the other operand): below 3 x 2^-35 + 2^-50 < 2^-33; ld multiplies, times two.  It matters only when one row sets the scale
           and the others sit 2^14 and more below it (their parts are f16 subnormals, or zero) - there the relative term alone is too
           small by orders of magnitude (tests/test_knn_wide_host.py shows it on the `outlier_q24` family).

"Clear" rows: with d(j) the j-th smallest float64 distance of a row and err in the distances' units (err / (sx sy)), a row is clear when
d(32) - d(k) > 4 err - the 32nd approximate value is within err of d(32), the refined k-th within less than err of d(k), and the proof
keeps 2 err between them: such a row has to be proven.  Conversely a row the proof passes has the oracle's top k among its candidates.
"""
import functools

import numpy as np

import distmat_x3_ref as x3
import matching_ref as mref

KK, CAP, KMAX, GROUPS = 32, 1024, 24, 32
NB_MIN, D_MIN, WIDE_MIN = 4096, 128, 1 << 25
oracle, select = mref.oracle, mref.select
METRIC_L2SQR = mref.METRIC_L2SQR


def ld_of(d):
    return (d + 63) // 64 * 64


def nbpad_of(n):
    return (n + 255) // 256 * 256


def err_scale(ld):
    return (6.0 * ld / 16.0 + 16.0) * 2.0 ** -24


def err_abs(ld):
    return ld * 2.0 ** -32


def row_err(r2, my, ss, ld, absolute=True):
    """The proof's bound per row in the matrix's units, from squared norms r2 [m], the largest squared gallery norm and ss = sx sy."""
    return err_scale(ld) * (np.asarray(r2, np.float64) + my) * ss + (err_abs(ld) if absolute else 0.0)


# ------------------------------------------------------------------------------------------------ scales
def pow2_inv(sq):
    """scale_prep_kernel's pow2_inv on the fp32 maximum of the squared norms."""
    sq = np.float32(sq)
    if not (sq > 0) or not (sq < np.inf):
        return 1.0
    _, e = np.frexp(np.sqrt(sq, dtype=np.float32))
    return float(2.0 ** -int(min(max(e, -100), 100)))


def sqnorms(a):
    a64 = np.asarray(a, np.float64)
    return (a64 * a64).sum(1)


def _fmax(v):
    """fmaxf over the row norms starting from 0: NaN is skipped, +inf wins."""
    v = np.asarray(v, np.float32)
    v = v[~np.isnan(v)]
    return np.float32(max(0.0, v.max())) if len(v) else np.float32(0.0)


def scales(x, y):
    """(sx, sy, sx sy, max |y|^2) from the float64 squared norms rounded to fp32 (the device sums them in fp32: where a maximum is not an
    exact fp32 sum the device's exponent may sit on the other side of a power of two - the GPU tests take the device's own sc)."""
    with np.errstate(over="ignore"):
        mx, my = _fmax(sqnorms(x).astype(np.float32)), _fmax(sqnorms(y).astype(np.float32))
    sx, sy = pow2_inv(mx), pow2_inv(my)
    return sx, sy, sx * sy, float(my)


# ------------------------------------------------------------------------------------------------ values
def true_values(x, y, ss):
    """float64 [m, n]: sx sy (|y|^2 - 2 x.y), what the candidate matrix approximates."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return ss * (sqnorms(y64)[None, :] - 2.0 * (x64 @ y64.T))


def candidate_matrix(x, y, sc=None):
    """The restated matrix in float64: the three-product dot of the scaled operands (scaling by a power of two is exact in fp32 short of
    underflow, which the clamp of the exponent to +-100 and fp32's range exclude for the families here) under the epilogue's formula."""
    sx, sy, ss, _ = sc if sc is not None else scales(x, y)
    xs, ys = np.asarray(x, np.float32) * np.float32(sx), np.asarray(y, np.float32) * np.float32(sy)
    return ss * sqnorms(y)[None, :] - 2.0 * x3.restate(xs, ys)[0]


def key32(v):
    """The order-preserving key of an fp32 value (-0 < +0)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def rowsel(mat32, ncols=None):
    """rowsel_kernel on an fp32 matrix [m, n] (columns past ncols are not looked at): keys uint64 [m, 32] = (key32 << 32 | column) ascending,
    ~0 where a row has fewer than 32 columns, the survivors per row, and overflow [m] (more than CAP survivors: the keys are then undefined)."""
    mat32 = np.ascontiguousarray(mat32, np.float32)
    m, n = mat32.shape
    n = n if ncols is None else ncols
    k32 = key32(mat32[:, :n]).astype(np.uint64)
    cols = np.arange(n, dtype=np.uint64)
    keys = np.full((m, KK), ~np.uint64(0), np.uint64)
    survivors = np.zeros(m, np.int64)
    for i in range(m):
        gmin = np.full(GROUPS, 0xffffffff, np.uint64)
        np.minimum.at(gmin, np.arange(n) % GROUPS, k32[i])
        live = k32[i] <= gmin.max()
        survivors[i] = live.sum()
        packed = np.sort((k32[i][live] << np.uint64(32)) | cols[live])[:KK]
        keys[i, :len(packed)] = packed
    return keys, survivors, survivors > CAP


def key_columns(keys):
    return (np.asarray(keys, np.uint64) & np.uint64(0xffffffff)).astype(np.int64)


def run(x, y, k, err_on=True, absolute=True, drop_tail=False, force_every=0, a=None):
    """The whole path restated on float64 values: (D, I, flagged [m], candidates [m, 32]).  err_on = False: the proof without its bound
    (err = 0); absolute = False: without err_abs; drop_tail: selection and fallback never look at the last n % 4 columns (the mutation
    of rowsel_kernel's ragged tail); a: a candidate matrix to use instead of the restated one."""
    m, n = x.shape[0], y.shape[0]
    sx, sy, ss, my = scales(x, y)
    ld = ld_of(x.shape[1])
    e = oracle(x, y, METRIC_L2SQR)
    r2 = sqnorms(x)
    with np.errstate(over="ignore"):
        whole = not (np.isfinite(r2.astype(np.float32)).all() and np.isfinite(sqnorms(y).astype(np.float32)).all())
    if whole:            # a squared norm that is NaN or +inf in fp32: the candidate stage is not consulted, every row is answered exactly
        D, I = select(e, k)
        return D, I, np.ones(m, bool), np.full((m, KK), -1, np.int64)
    a = candidate_matrix(x, y) if a is None else a
    ncols = n & ~3 if drop_tail else n
    keys, _, over = rowsel(a.astype(np.float32), ncols)
    err = row_err(r2, my, ss, ld, absolute) if err_on else np.zeros(m)
    cand = key_columns(keys)
    D = np.full((m, k), np.inf)
    I = np.full((m, k), -1, np.int32)
    flagged = over.copy()
    cols = np.arange(ncols)
    for i in range(m):
        if force_every > 0 and i % force_every == 0:
            flagged[i] = True
        c = cand[i][keys[i] != ~np.uint64(0)]
        best = c[np.lexsort((c, e[i, c]))][:k]
        if not flagged[i] and ncols > KK:
            a_last = np.float32(a[i, c[-1]]) if len(c) == KK else np.inf
            ek = (e[i, best[-1]] - r2[i]) * ss if len(best) == k else -np.inf
            flagged[i] = not (ek + err[i] < a_last - err[i])
        if flagged[i]:
            keep = ~np.isnan(e[i, :ncols])
            best = cols[keep][np.lexsort((cols[keep], e[i, :ncols][keep]))][:k]
        D[i, :len(best)], I[i, :len(best)] = e[i, best], best
    return D, I, flagged, cand


def clear_rows(x, y, k, absolute=True):
    """(clear [m], gap [m], 4 err [m]) in the distances' units."""
    sx, sy, ss, my = scales(x, y)
    s = np.sort(oracle(x, y, METRIC_L2SQR), axis=1)
    gap = s[:, KK - 1] - s[:, k - 1]
    four = 4.0 * row_err(sqnorms(x), my, ss, ld_of(x.shape[1]), absolute) / ss
    return gap > four, gap, four


def tied_rows(x, y, k):
    """Rows whose k-th and 32nd oracle values are equal: no proof can pass them."""
    s = np.sort(oracle(x, y, METRIC_L2SQR), axis=1)
    return s[:, k - 1] == s[:, KK - 1]


# ------------------------------------------------------------------------------------------------ operands
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def plain_operands(m, n, d, offset=0.0, seed=18):
    """N(0, 1) + offset without planted neighbours but one: y[n - 1] = x[m - 1], a zero distance in the last row and column.  Every row
    of TABLE has to be clear at offsets 0 and 10 (tests/test_knn_wide_host.py); at (300, 4099, 136), k = 24, offset 10 the smallest gap
    d(32) - d(24) of 300 rows lies near 4 err = 0.61, and about every other seed leaves one row below it - 18 keeps a factor 1.49."""
    rng = np.random.default_rng(seed + 1000003 * m + 1009 * n + d)
    x = (rng.normal(size=(m, d)) + offset).astype(np.float32)
    y = (rng.normal(size=(n, d)) + offset).astype(np.float32)
    y[n - 1] = x[m - 1]
    return _ro(x, y)


ROUNDED_FAMILIES = ("n01", "offset10", "scale2m13", "scale300", "outlier_q14", "outlier_q24", "outlier_y14", "zero_rows", "zero_queries",
                    "unit_max", "near_tie", "noisy_tie")


@functools.lru_cache(maxsize=None)
def rounded_family(name, m, n, d):
    """n01 / offset10: the plain rows; scale2m13 / scale300: times 2^-13 (squared norms near 2^-19: far inside f16's subnormals before the
    normalisation) / 300 (components beyond f16's 2^11-scaled range); outlier_q14 / outlier_q24: query 1 (0 when m = 1) times 2^14 /
    2^24 - it sets sx, and every other query's scaled parts are f16 subnormals / its high part is zero; outlier_y14: gallery row 5 times
    2^14; zero_rows: an all-zero query (the last but one, or the only one) and an all-zero gallery row 7; zero_queries: every query zero
    (max |x|^2 = 0: sx = 1); unit_max: rows times 2^-5 (norms below 1) and one unit vector on either side - maxima of exactly 1 = 2^0,
    so sx = sy = 2^-1; near_tie: matching_ref.rounded_operands - every seventh gallery row copies a query, some 65 zero distances per query
    at m = 9, more than the 32 candidates; noisy_tie: noisy_tie_operands below."""
    if name == "near_tie":
        return mref.rounded_operands(m, n, d, 0.0)
    if name == "noisy_tie":
        return noisy_tie_operands(m, n, d)[:2]
    x, y = (a.copy() for a in plain_operands(m, n, d, 10.0 if name == "offset10" else 0.0))
    q = min(1, m - 1)
    if name == "scale2m13":
        x, y = x * np.float32(2.0 ** -13), y * np.float32(2.0 ** -13)
    elif name == "scale300":
        x, y = x * np.float32(300.0), y * np.float32(300.0)
    elif name == "outlier_q14":
        x[q] *= np.float32(2.0 ** 14)
    elif name == "outlier_q24":
        x[q] *= np.float32(2.0 ** 24)
    elif name == "outlier_y14":
        y[5] *= np.float32(2.0 ** 14)
    elif name == "zero_rows":
        x[max(m - 2, 0)] = 0.0
        y[7] = 0.0
    elif name == "zero_queries":
        x[:] = 0.0
    elif name == "unit_max":
        x, y = x * np.float32(2.0 ** -5), y * np.float32(2.0 ** -5)
        x[q] = 0.0
        x[q, 3] = 1.0
        y[9] = 0.0
        y[9, 9] = -1.0
    elif name not in ("n01", "offset10"):
        raise ValueError(name)
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def noisy_tie_operands(m, n, d, near=40, seed=31):
    """The plain rows, and per query `near` = 40 gallery rows x_i (1 + 2^-20 u), u uniform in [-1, 1] per component: 40 distinct distances of
    about 2^-40 |x|^2, far below err and more of them than candidates.  Which 32 of the 40 the candidate stage keeps is up to its rounding,
    so the top k of the candidates is not the top k of the row: without the proof's bound a row comes back wrong.  (The copies of
    matching_ref.rounded_operands cannot show that: they are EXACT ties, which the column order resolves the same way in every arithmetic.)"""
    rng = np.random.default_rng(seed + n + d)
    x, y = (a.copy() for a in plain_operands(m, n, d))
    slots = rng.permutation(n - 1)[:m * near].reshape(m, near)
    for i in range(m):
        y[slots[i]] = (x[i].astype(np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, (near, d)))).astype(np.float32)
    return _ro(x, y, slots)


@functools.lru_cache(maxsize=None)
def identical_operands(m, n, d):
    """Every gallery row the same integer vector: every element of a row ties, all n survive the threshold (> CAP), columns 0 .. k - 1 win."""
    return mref.exact_operands(m, n, d, True)


@functools.lru_cache(maxsize=None)
def copies_operands(m, n, d, copies=1100, seed=23):
    """Exact family.  Query i is an integer vector v with component i moved by one (query 0 is v itself); v sits in `copies` gallery rows spread
    over the whole width, the last column among them: every query's nearest value (0 or 1) is tied `copies` > CAP times."""
    rng = np.random.default_rng(seed + n)
    y = rng.integers(-4, 5, (n, d)).astype(np.float32)
    v = rng.integers(-3, 4, d).astype(np.float32)
    x = np.tile(v, (m, 1))
    for i in range(1, m):
        x[i, i % d] += 1.0
    where = np.unique(np.concatenate([np.linspace(0, n - 1, copies).astype(np.int64), [n - 1]]))
    y[where] = v
    return _ro(x, y, where)


@functools.lru_cache(maxsize=None)
def straddle_operands(m, n, d, k, tied=40, seed=29):
    """Exact family.  Query i is an integer vector v_i of its own (entries -3 .. 3 at stride-spread positions); the gallery holds k - 1
    copies of it (distance 0) and `tied` rows v_i +- one unit in distinct components (distance 1 each, distinct rows): the k-th value is
    tied `tied` = 40 times, so the tie runs across the 32nd candidate.  Everything else is far (random integers: distance ~ 13 d)."""
    rng = np.random.default_rng(seed + n + k)
    y = rng.integers(-4, 5, (n, d)).astype(np.float32)
    x = rng.integers(-3, 4, (m, d)).astype(np.float32)
    slots = rng.permutation(n - 1)[:m * (k - 1 + tied)].reshape(m, k - 1 + tied)
    for i in range(m):
        y[slots[i, :k - 1]] = x[i]
        for t, j in enumerate(slots[i, k - 1:]):
            y[j] = x[i]
            y[j, t % d] += 1.0 if t % 2 else -1.0
    return _ro(x, y)


@functools.lru_cache(maxsize=None)
def nonfinite_family(name, m=9, n=4097, d=128):
    """nan: matching_ref.nonfinite_operands (a NaN with the sign clear in query 1, one with the sign set in gallery row 2, an all-zero query
    m - 1 and gallery row n - 1); inf: that, and one +inf component in gallery row 4; overflow: that, and query 3 times 1e20 - every
    component finite, the squared norm beyond fp32."""
    x, y = (a.copy() for a in mref.nonfinite_operands(m, n, d))
    if name == "inf":
        y[4, 1] = np.inf
    elif name == "overflow":
        x[3] *= np.float32(1e20)
    elif name != "nan":
        raise ValueError(name)
    return _ro(x, y)


NONFINITE_FAMILIES = ("nan", "inf", "overflow")

# ------------------------------------------------------------------------------------------------ shapes
# (nq, nb, d, k, why).  The smallest the path accepts: nb >= 4096, d >= 128; nbpad = 4352 for every nb here but 4096.
TABLE = (
    (9, 4096, 128, 5, "nb % 4 == 0: no ragged tail in rowsel_kernel, nbpad == nb; nq odd: one half-wave of refine_kernel without a row"),
    (9, 4097, 128, 1, "one tail column; k = 1: the proof compares the nearest value"),
    (9, 4097, 128, 5, "one tail column"),
    (9, 4097, 128, 24, "k = KMAX: eight candidates of margin"),
    (1, 4098, 128, 5, "two tail columns; one query: one block of rowsel, half a wave of refine"),
    (9, 4099, 136, 5, "three tail columns; d % 64 != 0: the padded copy, ld = 192"),
    (300, 4099, 136, 24, "two 256-row GEMM tiles, the second of 44 rows; 38 refine blocks, the last half used"),
    (300, 4351, 128, 20, "nbpad - nb = 1: the last GEMM column tile lacks one column; tail of three"),
)
# queries of the rounded families repeated to this many rows reach the fused fp32 search when the wide path is off (72 x 4097 >= 2^18)
FUSED_NQ = 72
NBS = tuple(sorted({r[1] for r in TABLE}))
# the edges of knn_wide_eligible: (nq, nb, d, k) pairs on either side, with knn_wide_min lowered to nq * nb of the FIRST of each pair
EDGES = (
    ((9, 4097, 128, 24), (9, 4097, 128, 25)),      # k <= 24
    ((9, 4096, 128, 5), (9, 4095, 128, 5)),        # nb >= 4096
    ((9, 4097, 128, 5), (9, 4097, 127, 5)),        # d >= 128
)
