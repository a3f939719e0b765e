"""numpy restatement of the selection with fp32-class candidates (csrc/select_x3.hip; reid_argmin_rows_x3*, reid_knn_x3*), shared by
tests/test_select_x3_host.py and tests/test_gpu_select_x3.py.  What is held to what: `pipeline` restates the device's decisions - the
threshold pass, the tile lists, the merge, T, the proof, the fallback - on a matrix of approximate values (tests/distmat_x3_ref.py's
`restate` through the float64 metric formulas) and a matrix of exact values (the float64 oracle), and has to return the plain
(value, column) selection of the exact matrix on every row; `bound_closed` restates the device's error bound B (bound_of) and is held
against the sum of the bounds tests/distmat_x3_ref.py and tests/matching_ref.py derive for the two entries.

The pipeline (per query row; KK = 32 candidates, C = KK keys per tile list, 128 column groups, a sample of the first max(512, n / 16) columns, in
whole tiles):
  thr0   the KK-th smallest, by (value, group), of the minima of the groups `column mod 128` over the sample: at least KK columns lie at
         or below it (every value passes when fewer than KK groups have a column);
  lists  per column tile (128 wide; 64 for n <= 64, one tile) the columns with value <= thr0, and of more than C of them the C
         smallest by (value, column): such a FULL list's last value bounds every column of the tile that it left out;
  merge  all listed keys by (value, column), ties to the lower column; the first KK are the candidates;
  T      min(thr0, every full list's last value, the first key the merge dropped): no column outside the candidates has a smaller approximate value;
  refine the candidates' exact values, the k smallest by (value, column);
  proof  n <= KK (every column is a candidate), or the k-th exact value < T - B, strictly; REID_METRIC_L2: T and B on the squared
         distance, the comparison after clamp and root;
  else   the k smallest of ALL exact values by (value, column).
"""
import functools

import numpy as np

import distmat_x3_ref as x3
import matching_ref as mref

METRIC_L2, METRIC_L2SQR, METRIC_COS_HALF, METRIC_COS, METRIC_DOT = range(5)
METRICS = x3.METRICS
KK, C, GROUPS, SAMPLE, KMAX = 32, 32, 128, 512, 24
# the shapes of the fp32-class matrix, and one with several column tiles past 2048 gallery rows
SHAPES = x3.SHAPES + ((40, 2100, 64),)
U, U16 = 2.0 ** -24, 2.0 ** -11


def tile_width(n):
    return 64 if n <= 64 else 128


def sample_of(n):
    """Columns the threshold pass looks at: the first 512, from 8192 columns on a sixteenth of them in whole 128-column tiles."""
    return min(n, max(SAMPLE, (n // 16 + 127) // 128 * 128))


# ------------------------------------------------------------------------------------------------ the bound
def bound_closed(metric, ld, xx, ymax, ymin):
    """bound_of (csrc/select_x3.hip) in float64: B for rows of squared norm xx [m], given the largest and smallest squared norm of y."""
    xx = np.asarray(xx, np.float64)
    a25, a36, tiny = 2.0 ** -25, 2.0 ** -36, 1.4e-45
    r, nx, ny = np.sqrt(float(ld)), np.sqrt(xx), np.sqrt(float(ymax))
    n3 = 3.0 * ld * 2.0 ** -23
    g3 = n3 / (1.0 - n3)
    ns = ((ld + 63) // 64 + 7) * U
    gs = ns / (1.0 - ns)
    dm = (ld + 4) * U
    with np.errstate(all="ignore"):
        if metric in (METRIC_COS, METRIC_COS_HALF):
            nymin = np.sqrt(float(ymin))
            qx, qy = r / nx, r / nymin
            lx = U16 + a25 * qx
            dx, hx = U16 * lx + a36 * qx, 1.0 + lx
            ly = U16 + a25 * qy
            dy, hy = U16 * ly + a36 * qy, 1.0 + ly
            e3r = dx * hy + hx * dy + lx * ly + g3 * (hx * hy + (lx + dx) * hy + hx * (ly + dy)) + tiny / (nx * nymin)
            eta = (1.0 + gs) * (1.0 + U) ** 3 - 1.0
            bq = (eta + e3r) / (1.0 - eta) * (1.0 + U) + U
            s = bq + U * (2.0 + bq) + dm * (nx / nymin + ny / nx + 2.0)
            return 1.25 * (s * 0.5 if metric == METRIC_COS_HALF else s)
        LX = U16 * nx + a25 * r
        DX, HX = U16 * LX + a36 * r, nx + LX
        LY = U16 * ny + a25 * r
        DY, HY = U16 * LY + a36 * r, ny + LY
        e3 = DX * HY + HX * DY + LX * LY + g3 * (HX * HY + (LX + DX) * HY + HX * (LY + DY)) + tiny
        s2 = (nx + ny) ** 2
        if metric == METRIC_DOT:
            return 1.25 * (e3 + dm * nx * ny)
        b2 = ((gs * (1.0 + U) + U) * (xx + ymax) + 2.0 * e3) * (1.0 + U) + U * s2
        bm = dm * s2
        if metric == METRIC_L2SQR:
            return 1.25 * (b2 + bm)
        w = 2.0 * b2 + 2e-12
        return 1.25 * (w + 3.0 * U * (s2 + w) + bm + 3.0 * U * (np.maximum(s2, 1e-12) + bm))


def summed_bounds(x, y, metric):
    """[m, n] float64: the bound tests/distmat_x3_ref.py derives for the fp32-class entry plus the one tests/matching_ref.py derives for
    the exact entry (REID_METRIC_L2: both on the square)."""
    return x3.oracle(x, y, metric)[1] + mref.bound(x, y, metric)


def row_bound(x, y, metric):
    """B per row of x as the device computes it: from the float64 squared norms (the device's fp32 norms differ by parts in 10^6, the
    factor 1.25 is there for that)."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    yy = (y64 * y64).sum(1)
    return bound_closed(metric, x3.ld_of(x64.shape[1]), (x64 * x64).sum(1), yy.max(), yy.min())


# ------------------------------------------------------------------------------------------------ values
def approx_values(x, y, metric):
    """The candidate stage's value in float64: the restated three-product dot through the metric formula (REID_METRIC_L2: the squared
    distance, as the device keeps it)."""
    dot = x3.restate(x, y)[0]
    if metric == METRIC_DOT:
        return dot
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rs, cq = (x64 * x64).sum(1)[:, None], (y64 * y64).sum(1)[None, :]
    if metric in (METRIC_L2, METRIC_L2SQR):
        return rs + cq - 2.0 * dot
    c = 1.0 - dot / (np.sqrt(rs) * np.sqrt(cq))
    return c if metric == METRIC_COS else c / 2.0


def final_of(metric, v):
    """The monotone map from the value the proof lives on to the value the entry returns."""
    return np.sqrt(np.maximum(v, 1e-12)) if metric == METRIC_L2 else v


def plain_select(e, k, higher=False):
    """The rule: per row the k smallest by (value, column), padded with (+inf, -1)."""
    m, n = e.shape
    D = np.full((m, k), np.inf)
    I = np.full((m, k), -1, np.int64)
    cols = np.arange(n)
    for i in range(m):
        order = np.lexsort((-cols if higher else cols, e[i]))[:k]
        D[i, :len(order)], I[i, :len(order)] = e[i][order], order
    return D, I


# ------------------------------------------------------------------------------------------------ the pipeline
def pipeline(a, e, k, B, metric=METRIC_L2SQR, ignore_bound=False, merged_only=False, higher=False, force_every=0):
    """a [m, n]: approximate values (REID_METRIC_L2: squared), e [m, n]: exact FINAL values, B [m].  Returns (D, I, recomputed [m] bool).
    Mutations: ignore_bound - the proof compares with T instead of T - B; merged_only - T comes from the merged list alone (the filter's
    threshold and the full tile lists' last values are forgotten); higher - ties go to the higher column, in the merge, the refinement and the fallback."""
    m, n = a.shape
    bn = tile_width(n)
    D = np.full((m, k), np.inf)
    I = np.full((m, k), -1, np.int64)
    redo = np.zeros(m, bool)
    cols = np.arange(n)
    sign = -1 if higher else 1
    for i in range(m):
        s = sample_of(n)
        gmin = np.full(GROUPS, np.inf)
        np.minimum.at(gmin, cols[:s] % GROUPS, a[i, :s])
        thr0 = np.sort(gmin)[KK - 1]                                  # +inf when fewer than KK groups have a column
        listed, full_last = [], np.inf
        for t0 in range(0, n, bn):
            passing = np.array([j for j in range(t0, min(n, t0 + bn)) if a[i, j] <= thr0], np.int64)
            passing = passing[np.lexsort((sign * passing, a[i, passing]))]
            if len(passing) > C:                                      # the list keeps the tile's C smallest; its last bounds the rest
                full_last = min(full_last, a[i, passing[C - 1]])
            listed += list(passing[:C])
        listed = np.array(listed, np.int64)
        order = listed[np.lexsort((sign * listed, a[i, listed]))]
        cand = order[:KK]
        dropped = a[i, order[KK]] if len(order) > KK else np.inf
        T = dropped if merged_only else min(thr0, full_last, dropped)
        best = cand[np.lexsort((sign * cand, e[i, cand]))][:k]
        proven = n <= KK or T == np.inf
        if not proven and len(best) == k:
            proven = bool(e[i, best[-1]] < final_of(metric, T if ignore_bound else T - B[i]))
        if force_every > 0 and i % force_every == 0:
            proven = False
        if not proven:
            best = np.lexsort((sign * cols, e[i]))[:k]
            redo[i] = True
        D[i, :len(best)], I[i, :len(best)] = e[i, best], best
    return D, I, redo


@functools.lru_cache(maxsize=None)
def float64_case(shape, metric, unit, k):
    """(x, y, clear [m], gap, bounds): the random family of tests/distmat_x3_ref.py on `shape`; clear[i] says that row i's float64 gap
    between its k-th and its (k + 8)-th smallest value exceeds 16 times the largest summed bound of the row (rows of a problem with fewer
    than k + 9 columns are clear: every column is a candidate there)."""
    x, y = x3.random_operands(*shape, unit=unit)
    n = y.shape[0]
    want = x3.oracle(x, y, metric)[0]            # REID_METRIC_L2: the square - the bounds live there too
    b = summed_bounds(x, y, metric).max(1)
    if n < k + 9:
        return x, y, np.ones(x.shape[0], bool), np.inf, b
    s = np.sort(want, axis=1)
    gap = s[:, k + 7] - s[:, k - 1]
    return x, y, gap > 16 * b, float(gap.min()), b


# ------------------------------------------------------------------------------------------------ adversarial operands
@functools.lru_cache(maxsize=None)
def adversarial_operands(negate=False, seed=31):
    """x [6, 64] and y [300, 64], unit rows.  Columns 10 and 140 of y are one vector, 37 and 290 another (different column tiles): exact
    ties, the lower column has to win; x[0] is the first of them and x[1] the second, so the tie is each row's minimum.  Rows 2 .. 5 of x
    each have 40 copies in y (columns 150 + 4 r + q mod 4 ...: spread over tiles 1 and 2) with 2^-20 relative noise per element: more
    near-ties than there are candidates, all closer to each other than B - such a row cannot be proven.  negate (REID_METRIC_DOT, whose minimum is the most
    OPPOSED column): the queries are returned negated, so that the same columns are each row's smallest values."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(6, 64))
    y = rng.normal(size=(300, 64))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    x, y = x.astype(np.float32), y.astype(np.float32)
    y[10] = y[140] = x[0]
    y[37] = y[290] = x[1]
    near = {}
    free = [j for j in range(300) if j not in (10, 140, 37, 290)]
    picks = rng.permutation(free)[:160].reshape(4, 40)
    for r in range(4):
        for j in picks[r]:
            y[j] = (x[2 + r].astype(np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, 64))).astype(np.float32)
        near[2 + r] = np.sort(picks[r])
    if negate:
        x = -x
    for a in (x, y):
        a.setflags(write=False)
    return x, y, near


@functools.lru_cache(maxsize=None)
def clustered_operands(per_id, m=40, n=2100, d=64, spread=0.25, seed=41):
    """A gallery SORTED BY IDENTITY: y's rows are `per_id` consecutive images of each identity (a unit centre plus `spread` times a unit
    noise vector, normalised), x has one further image of m of the identities.  A query's near columns are then neighbours, and so are those of every
    identity that resembles it: more of them than a tile list holds (C = 32) pass the filter inside one 128-column tile."""
    rng = np.random.default_rng(seed + per_id)
    ids = (n + per_id - 1) // per_id

    def unit(a):
        return a / np.linalg.norm(a, axis=-1, keepdims=True)
    centres = unit(rng.normal(size=(ids, d)))
    y = unit(centres[np.arange(n) // per_id] + spread * unit(rng.normal(size=(n, d))))
    who = rng.permutation(ids)[:m]
    x = unit(centres[who] + spread * unit(rng.normal(size=(m, d))))
    x, y = x.astype(np.float32), y.astype(np.float32)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, who
