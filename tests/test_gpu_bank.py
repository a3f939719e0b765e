"""The DeepSORT feature bank (csrc/bank.hip) kernel by kernel, against a float64 restatement of the metric.

Both cost kernels (bank_cost512_kernel for d = 512, bank_cost_kernel for every other d or with the `bank_fast` switch at 0), both
write paths of bank_update_impl (metadata as kernel arguments up to 128 writes, uploaded above), the wrap guard, clear and reuse,
the device entry points, non-finite input, and a tracker's cold start on the match stream.  Run on an MI355X: pytest -m gpu.

Error bound (derived from the fp32 error model, not from observed numbers).  u = 2^-24 is fp32's unit roundoff.  Every sum the
kernels form is a chain of at most n = ceil(d / 64) + 8 roundings: bank_cost_kernel's lanes add ceil(d / 64) products and a 6-level
shuffle tree adds the lanes; bank_cost512_kernel's lanes add 8 products and butterfly16 adds 6 levels; the write kernels' squared
norms add ceil(d / 256) terms per thread, 6 shuffle levels and 2 more.  A sum of n roundings is off by at most g_n * sum|terms|,
g_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1; an FMA only removes roundings).
  cosine, c = 1 - a.b / (|a| |b|):  the dot product is off by g_n sum|a_i b_i| <= g_n |a||b| (Cauchy-Schwarz), each squared norm
    by g_n of itself, so each square root by g_n / 2 + u; the product and the quotient add 2u, the subtraction from 1 another u |c|
    <= 2u.  |err| <= g_n (sum|a_i b_i| / (|a||b|) + 1) + 6u <= (2n + 6) u.
  squared euclidean, c = max(0, |a|^2 + |b|^2 - 2 a.b):  g_n |a|^2 + g_n |b|^2 + 2 g_n |a||b| <= 2 g_n (|a|^2 + |b|^2), the two
    additions add u (|a|^2 + |b|^2) and u |c| <= 2u (|a|^2 + |b|^2); the clamp is 1-Lipschitz.  |err| <= (2n + 3) u (|a|^2 + |b|^2).
  The minimum over a track's samples is off by at most the largest of its samples' errors.  Both bounds are multiplied by
  SAFETY = 2 for the second-order terms dropped above.  The float64 reference adds nothing at this scale.
A gated entry is compared with the reference's gate only where the reference lies more than GATE_BAND bounds from the gate.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import nn_matching as onm
from reid_amd import _ffi, synth, weights
from reid_amd._ffi import check

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SAFETY = 2.0
GATE_BAND = 3.0
COS, L2 = _ffi.METRIC_COS, _ffi.METRIC_L2SQR


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


# ----------------------------------------------------------------------------- float64 reference and bounds
class RefBank:
    """float64 DeepSORT metric: per-key sample lists truncated to the last `budget` (key = track id, or bank slot), with the ring
    position every held sample has on the device (the samples a key has received since it was last cleared, modulo budget)."""

    def __init__(self, budget):
        self.budget = budget
        self.samples, self.total = {}, {}

    def append(self, feats, keys):
        for f, k in zip(np.asarray(feats, np.float64), keys):
            k = int(k)
            self.samples[k] = (self.samples.get(k, []) + [f])[-self.budget:]
            self.total[k] = self.total.get(k, 0) + 1

    def clear(self, keys):
        for k in keys:
            self.samples.pop(int(k), None)
            self.total.pop(int(k), None)

    def partial_fit(self, feats, keys, active):
        self.append(feats, keys)
        self.clear([k for k in list(self.samples) if k not in set(active)])

    def count(self, k):
        return len(self.samples.get(int(k), []))

    def at_position(self, k, p):
        """The held sample of key k in ring position p."""
        held, total = self.samples[int(k)], self.total[int(k)]
        first = total - len(held)
        g = max(i for i in range(first, total) if i % self.budget == p)
        return held[g - first]

    def rows(self, k):
        if not self.samples.get(int(k)):
            raise KeyError(k)              # as the reference's metric: a target without samples has no cost row
        return np.stack(self.samples[int(k)])

    def cost(self, keys, dets, metric, max_distance=None):
        b = np.asarray(dets, np.float64)
        out = np.empty((len(keys), len(b)))
        for i, k in enumerate(keys):
            a = self.rows(k)
            dot = a @ b.T
            a2, b2 = (a * a).sum(1), (b * b).sum(1)
            if metric == COS:
                c = 1.0 - dot / np.sqrt(a2)[:, None] / np.sqrt(b2)[None, :]
            else:
                c = np.maximum(0.0, a2[:, None] + b2[None, :] - 2.0 * dot)
            out[i] = c.min(0)
        if max_distance is not None:                            # linear_assignment.min_cost_matching
            out[out > max_distance] = max_distance + 1e-5
        return out

    def bound(self, keys, dets, metric, d):
        """Per-entry error bound of the device cost (module docstring)."""
        n = -(-d // 64) + 8
        if metric == COS:
            return np.full((len(keys), len(dets)), SAFETY * (2 * n + 6) * U)
        b2 = (np.asarray(dets, np.float64) ** 2).sum(1)
        a2 = np.array([(self.rows(k) ** 2).sum(1).max() for k in keys])
        return SAFETY * (2 * n + 3) * U * (a2[:, None] + b2[None, :])


def gate32(max_distance):
    return np.float32(max_distance) + np.float32(1e-5)


def assert_close_to_ref(got, ref, keys, dets, metric, d, max_distance=None, what=""):
    """Ungated: |got - ref| <= bound everywhere.  Gated: the same below the gate, exactly the gate value above it, nothing within
    GATE_BAND bounds of the gate."""
    tol = ref.bound(keys, dets, metric, d)
    raw = ref.cost(keys, dets, metric)
    if max_distance is None:
        err = np.abs(got.astype(np.float64) - raw)
        w = np.unravel_index(np.argmax(err / tol), err.shape)
        assert np.all(err <= tol), "%s: error %.3g against a bound of %.3g at %s" % (what, err[w], tol[w], w)
        return
    below = raw < max_distance - GATE_BAND * tol
    above = raw > max_distance + GATE_BAND * tol
    assert np.all(np.abs(got[below] - raw[below]) <= tol[below]), what
    assert np.all(got[above] == gate32(max_distance)), what


def test_reference_restates_the_oracle_metric():
    """RefBank and oracle/nn_matching.py (fed float64) agree on one case with truncation past the budget and both metrics."""
    rng = np.random.default_rng(0)
    feats = rng.normal(0, 1, (23, 40))
    keys = [0, 1, 2, 1, 1, 0, 2, 2, 2, 2, 1, 0, 1, 1, 1, 2, 0, 0, 0, 0, 1, 2, 1]
    dets = rng.normal(0, 1, (9, 40))
    for metric, name in ((COS, "cosine"), (L2, "euclidean")):
        ref = RefBank(5)
        orc = onm.NearestNeighborDistanceMetric(name, 0.2, 5)
        ref.partial_fit(feats, keys, [0, 1, 2])
        orc.partial_fit(list(feats), keys, [0, 1, 2])
        want = orc.distance(dets, [2, 0, 1])
        np.testing.assert_allclose(ref.cost([2, 0, 1], dets, metric), want, rtol=0, atol=1e-12)
        thr = float(np.sort(want.ravel())[13:15].mean())      # between two entries: both sides decide alike
        np.testing.assert_allclose(ref.cost([2, 0, 1], dets, metric, thr), onm.gate(want, thr), rtol=0, atol=1e-12)
        with pytest.raises(KeyError):
            orc.distance(dets, [7])
        with pytest.raises(KeyError):
            ref.cost([7], dets, metric)


# ----------------------------------------------------------------------------- the device bank through the C ABI
class DevBank:
    def __init__(self, eng, max_tracks, budget, d):
        self.eng, self.lib, self.budget, self.d = eng, eng.lib, budget, d
        self.h = C.c_void_p()
        check(self.lib.reid_bank_create(eng.h, max_tracks, budget, d, C.byref(self.h)))

    def update(self, feats, slots):
        f = np.ascontiguousarray(feats, np.float32).reshape(-1, self.d)
        s = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_bank_update(self.eng.h, self.h, f.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), len(s)))

    def update_dev(self, d_feats, slots):
        s = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_bank_update_dev(self.eng.h, self.h, C.c_void_p(d_feats), s.ctypes.data_as(C.c_void_p), len(s)))

    def clear(self, slots):
        s = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_bank_clear(self.eng.h, self.h, s.ctypes.data_as(C.c_void_p), len(s)))

    def count(self, slot):
        n = C.c_int()
        check(self.lib.reid_bank_count(self.h, int(slot), C.byref(n)))
        return n.value

    def cost(self, slots, dets, metric, max_distance=None):
        s = np.ascontiguousarray(slots, np.int32)
        x = np.ascontiguousarray(dets, np.float32).reshape(-1, self.d)
        out = np.full((len(s), len(x)), np.nan, np.float32)
        check(self.lib.reid_bank_cost(self.eng.h, self.h, s.ctypes.data_as(C.c_void_p), len(s), x.ctypes.data_as(C.c_void_p), len(x),
                                      metric, C.c_float(-1.0 if max_distance is None else max_distance), out.ctypes.data_as(C.c_void_p)))
        return out

    def cost_dev(self, slots, d_dets, m, metric, max_distance, d_out):
        s = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_bank_cost_dev(self.eng.h, self.h, s.ctypes.data_as(C.c_void_p), len(s), C.c_void_p(d_dets), int(m), metric,
                                          C.c_float(-1.0 if max_distance is None else max_distance), C.c_void_p(d_out)))

    def close(self):
        self.eng.sync()
        self.lib.reid_bank_destroy(self.h)


class bank_fast:
    """Context manager: the d = 512 kernel choice (debug switch `bank_fast`), restored on the way out."""

    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.old = self.eng.debug_switch("bank_fast")
        self.eng.debug_switch("bank_fast", self.value)

    def __exit__(self, *exc):
        self.eng.debug_switch("bank_fast", self.old)


def _track_dirs(rng, n, d):
    return rng.normal(0, 1, (n, d)) * rng.uniform(0.5, 3.0, (n, 1))


def _fill(dev, ref, rng, totals, d, dirs, max_call=150):
    """Write totals[slot] samples to each slot, interleaved over calls of random size 1..max_call (both write paths)."""
    todo = [s for s, t in totals.items() for _ in range(t)]
    rng.shuffle(todo)
    i = 0
    while i < len(todo):
        k = int(rng.integers(1, max_call + 1))
        slots = np.asarray(todo[i:i + k], np.int32)
        feats = (dirs[slots] + rng.normal(0, 1.0, (len(slots), d))).astype(np.float32)
        dev.update(feats, slots)
        ref.append(feats, slots)
        i += k


def _dets(rng, ref, slots, m, d, dirs, special):
    """m detections: two in three are noisy copies of the sample in a chosen ring position of a track (positions around the
    kernels' wave strides and the last held row - a skipped row then costs ~1 instead of ~0), one in three a fresh vector."""
    out = np.empty((m, d), np.float32)
    keys = [s for s in slots if ref.count(s)]
    for j in range(m):
        if j % 3 == 2:
            out[j] = dirs[keys[j % len(keys)]] + rng.normal(0, 1.0, d)
            continue
        s = keys[j % len(keys)]
        cnt = ref.count(s)
        cand = sorted({p for p in special(cnt) if 0 <= p < cnt})
        p = cand[(j // len(keys)) % len(cand)] if j else cnt - 1
        base = ref.at_position(s, p)
        out[j] = base + rng.normal(0, [1e-3, 0.05, 0.3][(j + j // 3) % 3] * np.abs(base).mean(), d)
    return out


def _check_costs(dev, ref, slots, dets, metric, d, what):
    raw = dev.cost(slots, dets, metric)
    assert_close_to_ref(raw, ref, slots, dets, metric, d, None, what + " raw")
    rc = ref.cost(slots, dets, metric)
    thr = 0.15 if metric == COS else float(np.median(rc))
    gated = dev.cost(slots, dets, metric, thr)
    # the gate is the same kernel's last step: below it the raw value bit for bit, above it exactly max_distance + 1e-5
    np.testing.assert_array_equal(gated, np.where(raw > np.float32(thr), gate32(thr), raw))
    assert_close_to_ref(gated, ref, slots, dets, metric, d, thr, what + " gated")
    return raw


def _wave_positions(nw):
    return lambda cnt: [0, 1, nw - 1, nw, nw + 1, 2 * nw - 1, 2 * nw, cnt - nw - 1, cnt - nw, cnt - 2, cnt - 1]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("budget", [1, 7, 8, 9, 16, 17, 100, 130])
def test_cost512_kernel_against_float64(eng, budget, metric):
    """bank_cost512_kernel (d = 512, bank_fast = 1): tracks filled to totals below, at and past the budget (counts around its
    8-wave stride and past 2 budget, the wrap guard), in a shuffled slot order with a repeated slot; detection counts around the
    16-detection block."""
    d, rng = 512, np.random.default_rng(budget * 10 + metric)
    totals = {}
    for i, t in enumerate(sorted({1, 7, 8, 9, 16, 17, budget - 1, budget, budget + 1, 2 * budget + 1, 3 * budget + 2} - {0})):
        totals[3 * i + 1] = t                                  # slots 1, 4, 7, ...: not the first rows of the bank
    dirs = _track_dirs(rng, 3 * len(totals) + 2, d)
    dev, ref = DevBank(eng, 3 * len(totals) + 2, budget, d), RefBank(budget)
    try:
        with bank_fast(eng, 1):
            _fill(dev, ref, rng, totals, d, dirs)
            for s, t in totals.items():
                assert dev.count(s) == ref.count(s) == min(t, budget)
            slots = list(rng.permutation(list(totals))) + [list(totals)[-1]]
            for m in (1, 15, 16, 17, 33, 80):
                dets = _dets(rng, ref, slots, m, d, dirs, _wave_positions(8))
                _check_costs(dev, ref, slots, dets, metric, d, "budget %d m %d" % (budget, m))
    finally:
        dev.close()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d,fast", [(512, 0), (8, 1), (136, 1), (768, 1), (769, 1), (2048, 1)])
def test_generic_cost_kernel_against_float64(eng, d, fast, metric):
    """bank_cost_kernel: d = 512 with bank_fast = 0, and the other sizes (at 769 the launch starts to ask for more than 48 KB of
    dynamic LDS; 2048, the largest d reid_bank_create accepts, needs 128 KB).  Counts around its 16-wave stride."""
    budget, rng = 40, np.random.default_rng(d + 7 * metric)
    totals = {0: 1, 2: 15, 3: 16, 5: 17, 6: 33, 8: 39, 9: 40, 11: 41, 12: 81}
    dirs = _track_dirs(rng, 13, d)
    dev, ref = DevBank(eng, 13, budget, d), RefBank(budget)
    try:
        with bank_fast(eng, fast):
            _fill(dev, ref, rng, totals, d, dirs)
            slots = list(rng.permutation(list(totals)))
            for m in (1, 16, 17, 40):
                dets = _dets(rng, ref, slots, m, d, dirs, _wave_positions(16))
                _check_costs(dev, ref, slots, dets, metric, d, "d %d m %d" % (d, m))
    finally:
        dev.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_the_two_kernels_agree_at_d512(eng, metric):
    """Same bank, same detections: bank_cost512_kernel and bank_cost_kernel within the sum of their two bounds."""
    d, budget, rng = 512, 30, np.random.default_rng(3 + metric)
    totals = {0: 1, 1: 9, 2: 17, 3: 30, 4: 61}
    dirs = _track_dirs(rng, 5, d)
    dev, ref = DevBank(eng, 5, budget, d), RefBank(budget)
    try:
        _fill(dev, ref, rng, totals, d, dirs)
        dets = _dets(rng, ref, list(totals), 37, d, dirs, _wave_positions(8))
        with bank_fast(eng, 1):
            a = dev.cost(list(totals), dets, metric)
        with bank_fast(eng, 0):
            b = dev.cost(list(totals), dets, metric)
        tol = ref.bound(list(totals), dets, metric, d)
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * tol)
    finally:
        dev.close()


@pytest.mark.parametrize("fast", [1, 0])
def test_bound_survives_parallel_large_and_identical_inputs(eng, fast):
    """Nearly parallel vectors (cosine cost ~0), norms ~300 (the euclidean form cancels), and a detection equal to a stored sample:
    the clamped euclidean cost is >= 0 and within the bound of 0, the cosine cost within the bound of 0."""
    d, budget, rng = 512, 8, np.random.default_rng(17)
    base = rng.normal(0, 1, (4, d))
    base *= 300.0 / np.linalg.norm(base, axis=1, keepdims=True)
    base[0] /= 300.0                                                        # one unit-norm track
    feats = np.concatenate([base + rng.normal(0, s, base.shape) for s in (1e-4, 1e-3, 1e-2)]).astype(np.float32)
    slots = np.tile(np.arange(4), 3)
    dets = np.concatenate([feats[:4],                                       # identical to stored samples
                           (base + rng.normal(0, 1e-5, base.shape)).astype(np.float32),   # nearly parallel
                           (base * 1.0001).astype(np.float32)]).astype(np.float32)
    for metric in (COS, L2):
        dev, ref = DevBank(eng, 4, budget, d), RefBank(budget)
        try:
            with bank_fast(eng, fast):
                dev.update(feats, slots)
                ref.append(feats, slots)
                got = dev.cost(range(4), dets, metric)
            assert_close_to_ref(got, ref, list(range(4)), dets, metric, d)
            same = got[np.arange(4), np.arange(4)]
            tol = np.diag(ref.bound(list(range(4)), dets[:4], metric, d))
            assert np.all(np.abs(same) <= tol)
            if metric == L2:
                assert np.all(got >= 0)
        finally:
            dev.close()


# ----------------------------------------------------------------------------- write paths
def _same_bank(a, b, ra, slots, d, rng, dirs):
    dets = _dets(rng, ra, slots, 40, d, dirs, _wave_positions(8))
    for metric in (COS, L2):
        ca, cb = a.cost(slots, dets, metric), b.cost(slots, dets, metric)
        np.testing.assert_array_equal(ca, cb)
        assert_close_to_ref(ca, ra, slots, dets, metric, d)
    for s in slots:
        assert a.count(s) == b.count(s) == ra.count(s)


@pytest.mark.parametrize("spread", ["3 tracks", "129 tracks"])
def test_argument_and_uploaded_write_paths_leave_the_same_bank(eng, spread):
    """129 distinct writes in one call (uploaded metadata; with 129 tracks also more than 128 count updates) against 128 in one call
    (kernel arguments) followed by 1: identical counts and costs bit for bit, both within the bound of the reference."""
    d, budget, rng = 512, 64, np.random.default_rng(23)
    nt = 3 if spread == "3 tracks" else 129
    slots = np.arange(129, dtype=np.int32) % nt
    dirs = _track_dirs(rng, nt, d)
    feats = (dirs[slots] + rng.normal(0, 1, (129, d))).astype(np.float32)
    one, two = DevBank(eng, nt, budget, d), DevBank(eng, nt, budget, d)
    ref = RefBank(budget)
    try:
        one.update(feats, slots)
        two.update(feats[:128], slots[:128])
        two.update(feats[128:], slots[128:])
        ref.append(feats, slots)
        _same_bank(one, two, ref, list(range(nt)), d, rng, dirs)
    finally:
        one.close()
        two.close()


def test_one_call_wrapping_a_track_three_times(eng):
    """300 samples for one track in one call, budget 100: the argument path with 100 writes (a later sample replaces an earlier one
    at the same ring position) - the last 100 win."""
    d, budget, rng = 512, 100, np.random.default_rng(29)
    dirs = _track_dirs(rng, 2, d)
    feats = (dirs[[1] * 300] + rng.normal(0, 1, (300, d))).astype(np.float32)
    dev, ref = DevBank(eng, 2, budget, d), RefBank(budget)
    try:
        dev.update(feats, [1] * 300)
        ref.append(feats, [1] * 300)
        assert dev.count(1) == 100
        dets = np.concatenate([feats[[0, 99, 100, 199]], feats[[200, 250, 299]]])   # overwritten samples, then held ones
        for metric in (COS, L2):
            got = dev.cost([1], dets, metric)
            assert_close_to_ref(got, ref, [1], dets, metric, d)
            assert np.all(got[0, 4:] <= ref.bound([1], dets, metric, d)[0, 4:])
    finally:
        dev.close()


@pytest.mark.parametrize("budget", [1, 3, 10])
def test_wrap_guard_over_many_calls(eng, budget):
    """A track fed far past 2 budget in calls of 1..2 budget + 1 samples (reid_bank_update folds its total back into
    [budget, 2 budget)): after every call the count is min(total, budget) and the costs follow the reference."""
    d, rng = 512, np.random.default_rng(31 + budget)
    dirs = _track_dirs(rng, 2, d)
    dev, ref = DevBank(eng, 2, budget, d), RefBank(budget)
    try:
        total = 0
        for _ in range(12):
            k = int(rng.integers(1, 2 * budget + 2))
            feats = (dirs[[0] * k] + rng.normal(0, 1, (k, d))).astype(np.float32)
            dev.update(feats, [0] * k)
            ref.append(feats, [0] * k)
            total += k
            assert dev.count(0) == ref.count(0) == min(total, budget)
            dets = np.concatenate([feats[-min(k, budget):], dirs[:1] + rng.normal(0, 1, (3, d))]).astype(np.float32)
            for metric in (COS, L2):
                assert_close_to_ref(dev.cost([0], dets, metric), ref, [0], dets, metric, d, None, "total %d" % total)
        assert total > 2 * budget
    finally:
        dev.close()


def test_cleared_slot_reused_with_fewer_samples(eng):
    """A slot cleared and fed again with fewer samples than it held: the stale rows past the new count take no part."""
    d, budget, rng = 512, 16, np.random.default_rng(37)
    dirs = _track_dirs(rng, 3, d)
    old = (dirs[[2] * 12] + rng.normal(0, 1, (12, d))).astype(np.float32)
    new = (dirs[[2] * 3] + rng.normal(0, 1, (3, d))).astype(np.float32)
    dev, ref = DevBank(eng, 3, budget, d), RefBank(budget)
    try:
        dev.update(old, [2] * 12)
        dev.clear([2])
        dev.update(new, [2] * 3)
        ref.append(new, [2] * 3)
        assert dev.count(2) == 3
        dets = np.concatenate([old, new])
        for metric in (COS, L2):
            got = dev.cost([2], dets, metric)
            assert_close_to_ref(got, ref, [2], dets, metric, d)
            assert np.all(got[0, 3:12] > ref.bound([2], dets, metric, d)[0, 3:12] * 100)   # stale rows: no near-zero cost
    finally:
        dev.close()


@pytest.mark.parametrize("fast", [1, 0])
def test_track_without_samples(eng, fast):
    """A slot that holds no sample (never written, or cleared): max_distance + 1e-5 gated, inf raw.  The reference has no row for
    such a target (KeyError)."""
    d, rng = 512, np.random.default_rng(41)
    dev, ref = DevBank(eng, 3, 5, d), RefBank(5)
    try:
        feats = rng.normal(0, 1, (2, d)).astype(np.float32)
        dev.update(feats, [0, 2])
        ref.append(feats, [0, 2])
        dev.clear([2])
        ref.clear([2])
        dets = rng.normal(0, 1, (20, d)).astype(np.float32)
        with bank_fast(eng, fast):
            for metric in (COS, L2):
                raw, gated = dev.cost([1, 0, 2], dets, metric), dev.cost([1, 0, 2], dets, metric, 0.5)
                assert np.all(np.isinf(raw[[0, 2]])) and np.all(raw[[0, 2]] > 0)
                assert np.all(gated[[0, 2]] == gate32(0.5))
                assert_close_to_ref(raw[1:2], ref, [0], dets, metric, d)
        with pytest.raises(KeyError):
            ref.cost([1], dets, COS)
    finally:
        dev.close()


# ----------------------------------------------------------------------------- device entry points
@pytest.mark.parametrize("match_stream", [False, True])
def test_device_entry_points_equal_the_host_ones(eng, match_stream):
    """reid_bank_update_dev / reid_bank_cost_dev on reid_malloc'd buffers give the banks and costs of reid_bank_update /
    reid_bank_cost bit for bit (updates of both write paths), with the context's match stream off and on."""
    d, budget, rng = 512, 40, np.random.default_rng(43)        # 140 and 129 samples over 6 tracks: more than 128 distinct writes
    dirs = _track_dirs(rng, 6, d)
    calls = [rng.integers(0, 6, k).astype(np.int32) for k in (5, 140, 1, 60, 129)]
    dets = (dirs[rng.integers(0, 6, 33)] + rng.normal(0, 1, (33, d))).astype(np.float32)
    host, devb = DevBank(eng, 6, budget, d), DevBank(eng, 6, budget, d)
    ptrs = []
    eng.frame_match_stream(match_stream)
    try:
        d_feats = eng.malloc(140 * d * 4)
        d_dets = eng.malloc(dets.nbytes)
        d_out = eng.malloc(6 * 33 * 4)
        ptrs = [d_feats, d_dets, d_out]
        eng.h2d(d_dets, dets)
        for slots in calls:
            feats = (dirs[slots] + rng.normal(0, 1, (len(slots), d))).astype(np.float32)
            host.update(feats, slots)
            eng.device_sync()                     # the previous device update has read d_feats
            eng.h2d(d_feats, feats)
            devb.update_dev(d_feats, slots)
            for metric in (COS, L2):
                for gate in (None, 0.2 if metric == COS else 600.0):
                    want = host.cost(range(6), dets, metric, gate)
                    devb.cost_dev(list(range(6)), d_dets, 33, metric, gate, d_out)
                    got = eng.d2h(np.empty((6, 33), np.float32), d_out)
                    np.testing.assert_array_equal(got, want)
                    np.testing.assert_array_equal(devb.cost(range(6), dets, metric, gate), want)
        for s in range(6):
            assert host.count(s) == devb.count(s)
    finally:
        eng.device_sync()
        eng.frame_match_stream(False)
        for p in ptrs:
            eng.free(p)
        host.close()
        devb.close()


# ----------------------------------------------------------------------------- non-finite and zero-norm input
@pytest.mark.parametrize("fast", [1, 0])
def test_nan_and_zero_norm_rows_are_no_match(eng, fast):
    """The contract (reid_amd/nn_matching.py, distance): a sample whose cost against a detection is NaN - a NaN in either row, or a
    zero norm under the cosine metric - is left out of the minimum; where every sample of a track is such a row the entry is "no
    match" (inf raw, max_distance + 1e-5 gated), not NaN, and never a perfect match."""
    d, rng = 512, np.random.default_rng(47)
    feats = rng.normal(0, 1, (5, d)).astype(np.float32)
    feats[1, 7] = np.nan                                      # track 0: one good sample, one NaN sample
    feats[2, 3] = np.nan                                      # track 1: only a NaN sample
    feats[3] = 0.0                                            # track 2: only a zero sample
    slots = [0, 0, 1, 2, 3]                                   # track 3: one good sample
    dets = rng.normal(0, 1, (6, d)).astype(np.float32)
    dets[2, 100] = np.nan
    dets[4] = 0.0
    dev, ref = DevBank(eng, 4, 4, d), RefBank(4)
    ref.append(feats[[0, 4]], [0, 3])                         # the reference restricted to the finite samples
    good = [0, 1, 3, 5]
    try:
        dev.update(feats, slots)
        with bank_fast(eng, fast):
            for metric in (COS, L2):
                raw, gated = dev.cost([0, 1, 2, 3], dets, metric), dev.cost([0, 1, 2, 3], dets, metric, 0.5)
                assert not np.isnan(raw).any() and not np.isnan(gated).any()
                assert np.all(np.isinf(raw[1])) and np.all(raw[:, 2] == np.inf)          # NaN sample / NaN detection
                assert np.all(gated[1] == gate32(0.5)) and np.all(gated[:, 2] == gate32(0.5))
                assert_close_to_ref(raw[[0, 3]][:, good], ref, [0, 3], dets[good], metric, d)   # the NaN sample dropped
                if metric == COS:
                    assert np.all(raw[2] == np.inf) and np.all(raw[:, 4] == np.inf)       # zero norm: 0 / 0
                else:
                    zero = RefBank(4)
                    zero.append(feats[[3]], [2])
                    assert_close_to_ref(raw[2:3, good], zero, [2], dets[good], L2, d)
                    assert_close_to_ref(raw[[0, 3]][:, [4]], ref, [0, 3], dets[[4]], L2, d)
    finally:
        dev.close()


# ----------------------------------------------------------------------------- cold start of the stream classes
def _weights():
    sd = synth.seres18_state_dict(0)
    blob, manifest, _ = weights.pack_seres18(sd)
    return blob, manifest


class _Plan:
    """Track bookkeeping of one camera, independent of what the device returns: detection i of a frame feeds one of the live
    tracks, a spare detection starts a track (a new id, or one that died at least three frames before: reborn on a cleared slot),
    and every fifth frame the oldest track dies.  Tracks are born only through commit."""

    def __init__(self, base):
        self.alive, self.dead, self.next = [], [], base

    def commit(self, f, m):
        k = min(m, len(self.alive))
        rows = list(range(k))
        tg = [self.alive[(f + i) % len(self.alive)] for i in range(k)]
        if m > k and len(self.alive) < 6:
            back = [t for t, when in self.dead if when <= f - 3]
            if back:
                tid = back[0]
                self.dead = [(t, w) for t, w in self.dead if t != tid]
            else:
                tid, self.next = self.next, self.next + 1
            self.alive.append(tid)
            rows.append(k)
            tg.append(tid)
        if f % 5 == 4 and len(self.alive) > 1:
            self.dead.append((self.alive.pop(0), f))
        return rows, tg, list(self.alive)


MAXD, BUDGET, FRAMES = 0.2, 4, 30


def _frames(seed, n=FRAMES):
    pool = synth.ragged_crops_u8(24, seed=seed)
    sizes = np.random.default_rng(seed).integers(1, 7, n)
    return [[pool[(5 * f + i) % 24] for i in range(int(s))] for f, s in enumerate(sizes)]


def _run_camera(match_stream):
    from reid_amd.tracking import CameraStream
    blob, manifest = _weights()
    frames, plan, log = _frames(3), _Plan(100), []
    cam = CameraStream(blob, manifest, precision=0, max_dist=MAXD, budget=BUDGET, max_tracks=8, match_stream=match_stream)
    try:
        cam.submit(frames[0])                  # no partial_fit anywhere: the bank is created inside the first step
        for f, crops in enumerate(frames):
            targets = list(plan.alive)
            feats, cost, _ = cam.step(targets, None, None, frames[f + 1] if f + 1 < len(frames) else None)
            rows, tg, active = plan.commit(f, len(crops))
            cam.commit(rows, tg, active)
            log.append([(targets, feats.copy(), cost.copy(), rows, tg, active)])
    finally:
        cam.close(destroy=True)
    return log


def _run_multi(match_stream):
    from reid_amd.tracking import MultiCameraStream
    blob, manifest = _weights()
    frames, plans, log = [_frames(4), _frames(5)], [_Plan(100), _Plan(200)], []
    cams = MultiCameraStream(blob, manifest, 2, precision=0, max_dist=MAXD, budget=BUDGET, max_tracks=8, match_stream=match_stream)
    try:
        cams.submit([frames[0][0], frames[1][0]])
        for f in range(FRAMES):
            targets = [list(p.alive) for p in plans]
            nxt = [frames[0][f + 1], frames[1][f + 1]] if f + 1 < FRAMES else None
            res = cams.step(targets, None, None, nxt)
            plan = [p.commit(f, len(frames[c][f])) for c, p in enumerate(plans)]
            cams.commit([p[0] for p in plan], [p[1] for p in plan], [p[2] for p in plan])
            log.append([(targets[c], res[c][0].copy(), res[c][1].copy()) + tuple(plan[c]) for c in range(2)])
    finally:
        cams.close(destroy=True)
    return log


def _run_lookahead(match_stream):
    from reid_amd.tracking import LookaheadCameraStream
    blob, manifest = _weights()
    frames, plan, log = _frames(6), _Plan(100), []
    groups = [frames[i:i + 2] for i in range(0, FRAMES, 2)]
    s = LookaheadCameraStream(blob, manifest, frames_per_pass=2, precision=0, max_dist=MAXD, budget=BUDGET, max_tracks=8,
                              match_stream=match_stream)
    try:
        s.submit_group(groups[0])
        for g, group in enumerate(groups):
            for j, crops in enumerate(group):
                f = 2 * g + j
                targets = list(plan.alive)
                nxt = groups[g + 1] if j == s.handover and g + 1 < len(groups) else None
                feats, cost, _ = s.step(j, targets, None, None, next_group=nxt)
                rows, tg, active = plan.commit(f, len(crops))
                s.commit(j, rows, tg, active)
                log.append([(targets, feats.copy(), cost.copy(), rows, tg, active)])
    finally:
        s.close(destroy=True)
    return log


@pytest.mark.parametrize("run", [_run_camera, _run_multi, _run_lookahead], ids=["camera", "multi_camera", "lookahead"])
def test_cold_start_on_the_match_stream(run):
    """CameraStream, MultiCameraStream (2 cameras) and LookaheadCameraStream (F = 2) from an empty tracker - no host partial_fit at
    any point, so the bank is created inside the first step, after frame 0's forward was queued, and first fed by an update stage
    of the match stream - over 30 frames in which tracks are born only through commit, die and are reborn on cleared slots.
    Features and costs are the same bit for bit with match_stream on and off, and every frame's cost follows the float64 reference
    fed the committed features.

    What this can and cannot do: it pins the cold-start flow and the ordering of reid_bank_create's memset by construction (with the
    fix the memset is on the match stream, behind which every update and cost stage is queued).  Without the fix the outcome
    depended on a race whose window is a few microseconds behind frame 0's forward; a pass here does not show that race is gone,
    and this test is not meant to be looped to provoke it."""
    on, off = run(True), run(False)
    assert len(on) == len(off) == FRAMES
    compared = 0
    refs = None
    for f, (a, b) in enumerate(zip(on, off)):
        refs = refs or [RefBank(BUDGET) for _ in a]
        for c, ((targets, feats, cost, rows, tg, active), (_, feats_b, cost_b, _, _, _)) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(feats, feats_b)
            np.testing.assert_array_equal(cost, cost_b)
            assert cost.shape == (len(targets), len(feats))
            if targets:
                assert_close_to_ref(cost.astype(np.float32), refs[c], targets, feats, COS, 512, MAXD, "frame %d camera %d" % (f, c))
                compared += cost.size
            refs[c].partial_fit(feats[rows], tg, active)
    assert compared > 100
