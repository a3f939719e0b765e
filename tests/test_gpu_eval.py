"""The evaluation kernels against exact oracles: rank counting for CMC / mAP (select.hip rank_eval_kernel) and k-reciprocal
Jaccard re-ranking (rerank.hip).  Run on an MI355X: pytest -m gpu.

Rank counting.  The oracle is the reference's own compute_mAP (oracle/matching.py) fed with the good and junk sets of
evaluate_one and the order the library documents (reid_amd/evaluate.py): index = np.argsort(score, kind="stable")[::-1].
Features hold small integers (-3..3, d <= 64), so every dot product is an integer below 2^24 and exact in fp32 under any
summation order: the device's scores equal the float64 scores bit for bit, which each case asserts first (inf * 0 and
inf - inf give NaN in both).  With equal scores the ranks are equal, and AP is then summed in fp64 in the reference's own
order, so every comparison is exact: valid, the summed CMC and per-query AP with ==, and evaluate_all's mean mAP with ==.
The continuous-feature case at d = 512 ranks the scores eng.distmat(qf, gf, METRIC_DOT) returns, which is the call
reid_rank_eval_dev makes at the same shape (asserted on the source), so near-ties are exact too.

Re-ranking.  The oracle is oracle/rerank.compute_jaccard_distance from the same neighbour lists (exact float64 k-NN, self
included, ties by lower index; the library's own k-NN at n = 12 300).  Tolerance atol 3e-6, as in test_gpu_parity.py: the
integer steps are exact, the float steps are the reference's fp32 formulas summed in a different order (softmax denominator,
atomic min-sums) on values in [0, 1].  The two device paths are compared with each other at the same tolerance: each is one
more summation order of the same terms.  Every case runs with the `rerank_hbm_acc` debug switch off (accumulators in LDS
below 150 KB) and on (HBM scratch rows at every n), the latter twice on one context: the second call reuses the scratch.
At n = 12 300 (Jaccard accumulator and query-expansion LDS above 48 KB) the dense oracle is too slow; a row-restricted
restatement of it, checked against the dense one below, compares N_SAMPLE seeded rows.  N_SAMPLE = 64 is a chosen number,
not a measured one.
"""
import os
import re

import numpy as np
import pytest

from oracle import matching, rerank
from reid_amd import _ffi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ATOL = 3e-6
N_SAMPLE = 64
MAX_GOOD = 2048


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


# ----------------------------------------------------------------------------- rank counting: oracle
def ref_scores(qf, gf):
    """float64 similarity gf @ q for every query, elementwise (IEEE inf / NaN rules, no BLAS shortcuts), as float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.asarray(qf, np.float64)[:, None, :] * np.asarray(gf, np.float64)[None, :, :]).sum(-1)
    return s.astype(np.float32)


def oracle_one(score, ql, qc, gl, gc):
    """evaluate_one (reid/evaluate.py:55-75) with the documented stable order; compute_mAP is the reference's."""
    index = np.argsort(score, kind="stable")[::-1]
    query_index = np.argwhere(gl == ql)
    camera_index = np.argwhere(gc == qc)
    good_index = np.setdiff1d(query_index, camera_index, assume_unique=True)
    junk_index1 = np.argwhere(gl == -1)
    junk_index2 = np.intersect1d(query_index, camera_index)
    junk_index = np.append(junk_index2, junk_index1)
    return matching.compute_mAP(index, good_index, junk_index)


def oracle_all(scores, ql, qc, gl, gc):
    """(cmc_sum int64[ng], ap float64[nq] (0 when skipped), valid int32[nq], mean mAP) as reid/evaluate.py:33-52 sums them."""
    nq, ng = scores.shape
    cmc = np.zeros(ng, np.int64)
    ap = np.zeros(nq, np.float64)
    valid = np.zeros(nq, np.int32)
    total = 0.0
    for i in range(nq):
        ap_i, cmc_i = oracle_one(scores[i], ql[i], qc[i], gl, gc)
        if cmc_i[0] == -1:
            continue
        cmc += cmc_i
        ap[i] = ap_i
        valid[i] = 1
        total += ap_i
    return cmc, ap, valid, total / nq


def check_rank(eng, qf, ql, qc, gf, gl, gc, scores=None, what=""):
    from reid_amd.evaluate import evaluate_all
    ql, qc, gl, gc = (np.asarray(a, np.int64) for a in (ql, qc, gl, gc))
    if scores is None:
        scores = ref_scores(qf, gf)
        np.testing.assert_array_equal(eng.distmat(qf, gf, _ffi.METRIC_DOT), scores, err_msg=what + ": scores not exact")
    cmc_r, ap_r, valid_r, map_r = oracle_all(scores, ql, qc, gl, gc)
    cmc, ap, valid = eng.rank_eval(qf, ql, qc, gf, gl, gc)
    np.testing.assert_array_equal(valid != 0, valid_r != 0, err_msg=what + ": valid")
    np.testing.assert_array_equal(cmc, cmc_r, err_msg=what + ": summed CMC")
    bad = np.flatnonzero(ap != ap_r)
    assert bad.size == 0, "%s: per-query AP differs at %s: %s against %s" % (what, bad[:8], ap[bad[:8]], ap_r[bad[:8]])
    cmc_e, map_e = evaluate_all(qf, ql, qc, gf, gl, gc, verbose=False)
    assert map_e == map_r, (what, map_e, map_r)
    np.testing.assert_array_equal(np.asarray(cmc_e), cmc_r.astype(np.float32) / len(ql), err_msg=what)
    return valid_r


def int_feats(rng, n, d, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, (n, d)).astype(np.float32)


# ----------------------------------------------------------------------------- rank counting: cases
def test_rank_oracle_restates_reference_evaluate_all():
    """Without ties the stable order is np.argsort's: oracle_all equals oracle/matching.evaluate_all on continuous features."""
    qf, ql, qc, gf, gl, gc = synth.clustered_embeddings(20, 400, d=32, n_ids=15, n_cams=3, seed=7)
    gl[::17] = -1
    cmc_r, _, _, map_r = oracle_all(ref_scores(qf, gf), ql, qc, gl, gc)
    cmc_m, map_m = matching.evaluate_all(qf, ql, qc, gf, gl, gc)
    np.testing.assert_array_equal(cmc_r.astype(np.float32) / 20, cmc_m)
    assert abs(map_r - map_m) < 1e-12


def test_rank_many_exact_ties(eng):
    """Duplicate gallery rows (40 distinct rows among 300), queries along one axis (seven score levels), a zero query (one
    level, -0 and +0 alike) and queries orthogonal to most of the gallery."""
    rng = np.random.default_rng(1)
    d = 24
    base = int_feats(rng, 40, d)
    base[:30, :8] = 0                                        # 30 of the 40 rows are orthogonal to e_0..e_7
    gf = base[rng.integers(0, 40, 300)]
    gl = rng.integers(0, 6, 300)
    gc = rng.integers(0, 3, 300)
    qf = int_feats(rng, 14, d)
    qf[0] = 0
    qf[0, 0] = 2                                             # 2 * g[:, 0]
    qf[1] = 0                                                # every score 0
    qf[2] = 0
    qf[2, :8] = rng.integers(-3, 4, 8)                       # orthogonal to most of the gallery
    qf[3] = -qf[2]
    ql = rng.integers(0, 6, 14)
    qc = rng.integers(0, 3, 14)
    assert check_rank(eng, qf, ql, qc, gf, gl, gc, what="ties").sum() >= 10


def test_rank_ties_straddle_good_junk_and_plain(eng):
    """Five distinct gallery rows: every score level holds good items, same-camera junk, -1 junk and other ids."""
    rng = np.random.default_rng(2)
    d = 16
    base = int_feats(rng, 5, d)
    ng = 400
    gf = base[rng.integers(0, 5, ng)]
    gl = rng.choice(np.array([-1, 1, 2, 3]), ng)
    gc = rng.integers(0, 3, ng)
    qf = np.concatenate([base, int_feats(rng, 7, d)])
    ql = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3])
    qc = rng.integers(0, 3, 12)
    scores = ref_scores(qf, gf)
    for i in range(12):                                      # the cases are what the test says they are
        for lvl in np.unique(scores[i]):
            at = scores[i] == lvl
            good = at & (gl == ql[i]) & (gc != qc[i])
            junk = at & ((gl == -1) | ((gl == ql[i]) & (gc == qc[i])))
            assert good.any() and junk.any() and (at & ~good & ~junk).any()
    assert check_rank(eng, qf, ql, qc, gf, gl, gc, what="straddle").all()


def test_rank_junk_labels_and_skipped_queries(eng):
    """Gallery label -1 in the query's camera and in others; a query whose same-id items all lie in its own camera (valid 0,
    still counted in the denominator); a query id absent from the gallery; a query labelled -1 whose -1 items are all in its
    own camera (valid 0)."""
    rng = np.random.default_rng(3)
    d, ng = 32, 500
    gf = int_feats(rng, ng, d)
    gl = rng.integers(0, 8, ng)
    gc = rng.integers(0, 4, ng)
    gl[rng.random(ng) < 0.2] = -1
    gl[(gl == -1) & (gc != 2)] = 0                           # label -1 only in camera 2 (see the -1 query below)
    gl[gl == 5] = 6
    gl[(gl == 7) & (gc != 1)] = 6                            # id 7: camera 1 only
    assert ((gl == -1) & (gc == 2)).any() and (gl == 7).any()
    qf = int_feats(rng, 10, d)
    ql = np.array([1, 2, 3, 7, 5, -1, 4, 6, 0, 2])
    qc = np.array([2, 0, 1, 1, 0, 2, 3, 2, 1, 2])
    valid = check_rank(eng, qf, ql, qc, gf, gl, gc, what="junk")
    np.testing.assert_array_equal(valid, [1, 1, 1, 0, 0, 0, 1, 1, 1, 1])


def test_rank_all_junk_gallery(eng):
    rng = np.random.default_rng(4)
    gf = int_feats(rng, 300, 20)
    gc = rng.integers(0, 3, 300)
    gl = np.where(rng.random(300) < 0.5, -1, 1 + gc)         # id c + 1 lives in camera c only
    qf = int_feats(rng, 6, 20)
    ql = np.array([1, 2, 3, 1, 2, 3])
    qc = np.array([0, 1, 2, 0, 1, 2])
    valid = check_rank(eng, qf, ql, qc, gf, gl, gc, what="all junk")
    assert not valid.any()


@pytest.mark.parametrize("nq,ng", [(5, 1), (5, 3), (5, 255), (5, 256), (5, 257), (5, 1000), (1, 257)])
def test_rank_gallery_sizes(eng, nq, ng):
    """Galleries below, at and above one 256-thread block; one query alone."""
    rng = np.random.default_rng(100 + ng + nq)
    d = 13
    gf = int_feats(rng, ng, d, -1, 1)                        # few score levels: ties at every size
    gl = rng.integers(0, 3, ng)
    gc = rng.integers(0, 2, ng)
    if ng > 3:
        gl[rng.random(ng) < 0.1] = -1
    gl[0], gc[0] = 1, 1                                      # every size has a good item for query 0
    qf = int_feats(rng, nq, d, -1, 1)
    ql = np.ones(nq, np.int64)
    qc = np.zeros(nq, np.int64)
    assert check_rank(eng, qf, ql, qc, gf, gl, gc, what="ng %d" % ng)[0] == 1


@pytest.mark.parametrize("ngood", [MAX_GOOD, MAX_GOOD + 1])
def test_rank_max_good(eng, ngood):
    """Exactly 2048 good items are counted; 2049 are refused with an error naming the query."""
    rng = np.random.default_rng(5)
    ng = ngood + 300
    gf = int_feats(rng, ng, 8, -2, 2)
    gl = np.concatenate([np.full(ngood, 7), rng.integers(0, 5, 300)])
    gc = np.concatenate([np.ones(ngood, np.int64), rng.integers(0, 3, 300)])
    gl[ngood:][gl[ngood:] == 0] = -1
    qf = int_feats(rng, 3, 8, -2, 2)
    ql = np.array([1, 7, 2])
    qc = np.array([0, 0, 1])
    if ngood <= MAX_GOOD:
        assert check_rank(eng, qf, ql, qc, gf, gl, gc, what="2048 good").all()
    else:
        with pytest.raises(_ffi.ReidHipError, match="query 1 "):
            eng.rank_eval(qf, ql, qc, gf, gl, gc)


def test_rank_non_finite_scores(eng):
    """+-inf and NaN feature entries: inf, -inf and NaN score columns (inf * 0 is NaN), NaN ranked first and NaN ties by higher
    gallery index first, as numpy's reversed stable argsort orders them; NaN columns among good, junk and plain items."""
    rng = np.random.default_rng(6)
    d, ng = 16, 600
    gf = int_feats(rng, ng, d, -2, 2)
    gl = rng.integers(0, 4, ng)
    gc = rng.integers(0, 3, ng)
    gl[rng.random(ng) < 0.1] = -1
    rows = rng.choice(ng, 90, replace=False)
    gf[rows[:30], 0] = np.inf
    gf[rows[30:50], 1] = -np.inf
    gf[rows[50:60], 0] = np.inf
    gf[rows[50:60], 1] = np.inf
    gf[rows[60:75], 2] = np.nan
    gf[rows[75:90], 0] = np.inf
    gf[rows[75:90], 2] = -np.inf                            # inf - inf
    qf = int_feats(rng, 16, d, -2, 2)
    qf[:4, 0] = 0                                           # inf * 0 = NaN for the first four queries
    qf[4:8, 0] = 1
    qf[8:12, 1] = -1
    qf[12:, 2] = 0
    ql = rng.integers(0, 4, 16)
    qc = rng.integers(0, 3, 16)
    scores = ref_scores(qf, gf)
    assert np.isnan(scores).any(axis=1).all() and np.isposinf(scores).any() and np.isneginf(scores).any()
    assert check_rank(eng, qf, ql, qc, gf, gl, gc, what="non-finite").sum() >= 12


def test_rank_unlabelled_query_with_unlabelled_items_in_other_cameras_is_refused(eng):
    """Items labelled -1 in another camera than a query labelled -1 are good and junk at once (the reference raises
    IndexError): refused with an error naming the query, whether the -1 items lie in one camera or in several."""
    rng = np.random.default_rng(8)
    gf = int_feats(rng, 50, 8)
    gc = rng.integers(0, 3, 50)
    gl = rng.integers(0, 4, 50)
    qf = int_feats(rng, 3, 8)
    ql = np.array([1, 2, -1])
    gl[5], gc[5] = -1, 2
    with pytest.raises(_ffi.ReidHipError, match="query 2 "):
        eng.rank_eval(qf, ql, np.array([0, 1, 1]), gf, gl, gc)   # -1 items in camera 2 only, the -1 query in camera 1
    valid = check_rank(eng, qf, ql, np.array([0, 1, 2]), gf, gl, gc, what="-1 query, own camera")
    assert valid[2] == 0
    gl[6], gc[6] = -1, 0                                         # -1 items in cameras 0 and 2: every -1 query is refused
    with pytest.raises(_ffi.ReidHipError, match="query 2 "):
        eng.rank_eval(qf, ql, np.array([0, 1, 2]), gf, gl, gc)


def test_rank_continuous_market_width(eng):
    """d = 512 clustered embeddings, Market-like labels: the oracle ranks the device's own similarity matrix."""
    src = open(os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc", "api.hip")).read()
    body = src[src.index("int reid_rank_eval_dev("):]
    body = body[:body.index("\n}\n")]
    calls = re.findall(r"reid_distmat_dev\(([^()]*)\)", body)
    assert calls == ["ctx, d_qf, nq, d_gf, ng, d, REID_METRIC_DOT, score"], calls
    host = src[src.index("int reid_distmat(reid_ctx*"):]
    host = host[:host.index("\n}\n")]
    assert re.findall(r"reid_distmat_dev\(([^()]*)\)", host) == ["ctx, io.dx, m, io.dy, n, d, metric, d_out"]
    assert "io.upload(qf, nq, gf, ng, d)" in src and "io.upload(x, m, y, n, d)" in src
    qf, ql, qc, gf, gl, gc = synth.clustered_embeddings(150, 4000, d=512, n_ids=100, n_cams=6, seed=9)
    gl[::23] = -1
    scores = eng.distmat(qf, gf, _ffi.METRIC_DOT)
    np.testing.assert_array_equal(eng.distmat(qf, gf, _ffi.METRIC_DOT), scores)          # deterministic
    assert np.abs(scores - qf.astype(np.float64) @ gf.astype(np.float64).T).max() < 1e-5  # and the dot product it claims
    assert check_rank(eng, qf, ql, qc, gf, gl, gc, scores=scores, what="market width").sum() > 100


# ----------------------------------------------------------------------------- re-ranking: oracles
def knn_rank(x, k):
    """Exact k-NN of every row (float64 squared L2, self included, ties by lower index) as int32 [n, k]."""
    x = np.asarray(x, np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


def unit_rows(rng, n, d, dup=0):
    """L2-normalised float32 rows; `dup` of them copies of earlier rows (a later copy's nearest neighbour is not itself)."""
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    if dup:
        src = rng.integers(0, n // 2, dup)
        dst = rng.choice(np.arange(n // 2, n), dup, replace=False)
        x[dst] = x[src]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def jaccard_rows(x, rank, k1, k2, rows):
    """compute_jaccard_distance restricted to `rows`, from sparse rows: V from the oracle's own sparse_v, the query expansion
    summed row by row in float32 as np.mean over axis 0 does, each output row accumulated column by column in ascending order
    as the dense oracle does."""
    n = x.shape[0]
    v = rerank.sparse_v(x, rank, k1)
    if k2 != 1:
        ke = min(k2, rank.shape[1])
        vq = []
        for i in range(n):
            src = [v[r] for r in rank[i, :ke]]
            idx = np.unique(np.concatenate([e for e, _ in src]))
            acc = np.zeros(len(idx), np.float32)
            for e, w in src:
                acc[np.searchsorted(idx, e)] += w
            vq.append((idx, (acc / np.float32(ke)).astype(np.float32)))
        v = vq
    ri = np.concatenate([np.full(len(e), i) for i, (e, _) in enumerate(v)])
    ci = np.concatenate([e for e, _ in v])
    vi = np.concatenate([w for _, w in v])
    order = np.argsort(ci, kind="stable")
    ri, ci, vi = ri[order], ci[order], vi[order]
    start = np.searchsorted(ci, np.arange(n + 1))
    out = np.zeros((len(rows), n), np.float32)
    for o, i in enumerate(rows):
        tmin = np.zeros(n, np.float32)
        e, w = v[i]
        for c, vic in zip(e, w):
            js = ri[start[c]:start[c + 1]]
            tmin[js] = tmin[js] + np.minimum(vic, vi[start[c]:start[c + 1]])
        out[o] = 1 - tmin / (2 - tmin)
    out[out < 0] = 0.0
    return out


def run_both_paths(eng, x, k1, k2, rank, want, rows=None, what=""):
    """Device Jaccard with the LDS accumulators (switch off) and the HBM scratch rows (switch on, twice on one context)."""
    outs = []
    try:
        for hbm, calls in ((0, 1), (1, 2)):
            eng.debug_switch("rerank_hbm_acc", hbm)
            for c in range(calls):
                got = eng.rerank_jaccard(x, k1, k2, rank=rank)
                sub = got if rows is None else got[rows]
                err = np.abs(sub - want)
                w = np.unravel_index(np.argmax(err), err.shape)
                assert err.max() <= RR_ATOL, "%s, rerank_hbm_acc %d, call %d: error %.3g at %s" % (what, hbm, c, err[w], w)
                assert (got >= 0).all() and (got <= 1).all()
            outs.append(got)
    finally:
        eng.debug_switch("rerank_hbm_acc", 0)
    return outs


# ----------------------------------------------------------------------------- re-ranking: cases
def test_row_oracle_restates_dense_oracle():
    rng = np.random.default_rng(11)
    for n, k1, k2 in ((120, 9, 4), (90, 5, 1), (60, 1, 3)):
        x = unit_rows(rng, n, 8, dup=6)
        rank = knn_rank(x, k1)
        want = rerank.compute_jaccard_distance(x, k1, k2, initial_rank=rank)
        rows = rng.choice(n, 20, replace=False)
        np.testing.assert_array_equal(jaccard_rows(x, rank, k1, k2, rows), want[rows])


# n, d, k1, k2, duplicated rows.  kh = round(k1 / 2) half to even, kh1 = min(kh + 1, k1), w1 = k1 + k1 kh1,
# w2 = min(min(k2, k1) w1, n); persistent grid = min(n, 2 x 256 CUs)
RR_CASES = [
    (300, 16, 64, 6, 0),     # k1 = MAX_K1 (full wave in recip_kernel), w2 clamped to n
    (64, 8, 64, 6, 4),       # k1 = n = MAX_K1
    (50, 8, 50, 2, 0),       # k1 = n
    (100, 8, 1, 1, 10),      # k1 = 1: kh = round(0.5) = 0, no query expansion
    (100, 8, 1, 3, 10),      # k1 = 1 < k2: expansion over one neighbour, which is not the row itself for later duplicates
    (257, 12, 9, 4, 0),      # kh = round(4.5) = 4
    (257, 12, 11, 3, 0),     # kh = round(5.5) = 6
    (200, 8, 5, 9, 6),       # k2 > k1: clamped to k1
    (1000, 16, 5, 2, 0),     # w2 = 2 w1 = 40 < n; grid 512 < n: blocks take several rows
    (1100, 16, 20, 6, 0),    # default k: n > 1024, not a multiple of 1024 (col_scan_kernel)
    (700, 16, 20, 1, 0),     # default k1 without query expansion
]


@pytest.mark.parametrize("n,d,k1,k2,dup", RR_CASES, ids=["n%d_k%d_%d%s" % (c[0], c[2], c[3], "_dup" if c[4] else "") for c in RR_CASES])
def test_rerank_edges_against_dense_oracle(eng, n, d, k1, k2, dup):
    rng = np.random.default_rng(n * 131 + k1 * 7 + k2)
    x = unit_rows(rng, n, d, dup)
    rank = knn_rank(x, k1)
    want = rerank.compute_jaccard_distance(x, k1, k2, initial_rank=rank)
    run_both_paths(eng, x, k1, k2, rank, want, what="n %d k1 %d k2 %d" % (n, k1, k2))


def test_rerank_above_48k_lds_against_row_oracle(eng):
    """n = 12 300: the Jaccard accumulator (n * 4 B) and the query expansion's (w2 + n) * 4 B both take the dynamic-LDS
    launches above 48 KB; the same n with the HBM scratch rows; N_SAMPLE seeded rows against the row-restricted oracle."""
    n, d, k1, k2 = 12300, 16, 20, 6
    assert n * 4 > 48 * 1024 and (6 * (20 + 20 * 11) + n) * 4 > 48 * 1024 and (6 * 240 + n) * 4 <= 150 * 1024
    rng = np.random.default_rng(12)
    x = unit_rows(rng, n, d)
    _, rank = eng.knn(x, x, k1)
    rows = np.sort(rng.choice(n, N_SAMPLE, replace=False))
    want = jaccard_rows(x, rank, k1, k2, rows)
    lds, hbm = run_both_paths(eng, x, k1, k2, rank, want, rows=rows, what="n 12300")
    for lo in range(0, n, 2048):                                  # the two paths agree everywhere
        assert np.abs(lds[lo:lo + 2048] - hbm[lo:lo + 2048]).max() <= RR_ATOL, lo
