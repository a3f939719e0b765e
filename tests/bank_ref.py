"""float64 restatement of the DeepSORT appearance metric with a ring-buffer bank, and the error bounds of the device cost kernels
(csrc/bank.hip, csrc/bank96.hip), shared by tests/test_frame_swin_host.py and tests/test_gpu_frame_swin.py.  It restates the reference
and the bounds of tests/test_gpu_bank.py's docstring with the chain length n as a parameter.

Error bound (derived from the fp32 error model, not from observed numbers).  u = 2^-24 is fp32's unit roundoff.  Every sum a kernel
forms is a chain of at most n roundings, and a sum of n roundings is off by at most g_n * sum|terms|, g_n = n u / (1 - n u) (Higham,
Accuracy and Stability of Numerical Algorithms, 3.1; an FMA only removes roundings).
  cosine, c = 1 - a.b / (|a| |b|):  the dot product is off by g_n sum|a_i b_i| <= g_n |a||b| (Cauchy-Schwarz), each squared norm by
    g_n of itself, so each square root by g_n / 2 + u; the product and the quotient add 2u, the subtraction from 1 another u |c| <= 2u.
    |err| <= g_n (sum|a_i b_i| / (|a||b|) + 1) + 6u <= (2n + 6) u.
  squared euclidean, c = max(0, |a|^2 + |b|^2 - 2 a.b):  g_n |a|^2 + g_n |b|^2 + 2 g_n |a||b| <= 2 g_n (|a|^2 + |b|^2), the two
    additions add u (|a|^2 + |b|^2) and u |c| <= 2u (|a|^2 + |b|^2); the clamp is 1-Lipschitz.  |err| <= (2n + 3) u (|a|^2 + |b|^2).
  The minimum over a track's samples is off by at most the largest of its samples' errors.  Both bounds are multiplied by SAFETY = 2 for
  the second-order terms dropped above.  The float64 reference adds nothing at this scale.
A gated entry is compared with the reference's gate only where the reference lies more than GATE_BAND bounds from the gate.

Chain lengths:
  chain_generic(d) = ceil(d / 64) + 8   bank_cost_kernel: a lane adds ceil(d / 64) products, a 6-level shuffle tree adds the lanes; the
                                        write kernels' squared norms add ceil(d / 256) terms per thread, 6 levels and 2 more.
  CHAIN_96 = 6 + 4                      bank_cost96_kernel: a lane adds 6 products (dot product and the detection's squared norm alike),
                                        a 4-level butterfly adds the 16 lanes of a group.  The samples' squared norms come from the
                                        write kernels: 1 + 6 + 2 = 9 roundings at d = 96, inside the same n.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
GATE_BAND = 3.0
COS, L2 = 3, 1               # reid_amd._ffi.METRIC_COS / METRIC_L2SQR (include/reid_hip.h), checked by the host test
CHAIN_96 = 6 + 4


def chain_generic(d):
    return -(-d // 64) + 8


class RefBank:
    """float64 DeepSORT metric: per-key sample lists truncated to the last `budget` (key = track id, or bank slot)."""

    def __init__(self, budget):
        self.budget = budget
        self.samples = {}

    def append(self, feats, keys):
        for f, k in zip(np.asarray(feats, np.float64), keys):
            k = int(k)
            self.samples[k] = (self.samples.get(k, []) + [f])[-self.budget:]

    def clear(self, keys):
        for k in keys:
            self.samples.pop(int(k), None)

    def partial_fit(self, feats, keys, active):
        self.append(feats, keys)
        self.clear([k for k in list(self.samples) if k not in set(active)])

    def count(self, k):
        return len(self.samples.get(int(k), []))

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

    def bound(self, keys, dets, metric, n):
        """Per-entry error bound of a device cost whose sums are chains of at most n roundings (module docstring)."""
        if metric == COS:
            return np.full((len(keys), len(dets)), SAFETY * (2 * n + 6) * U)
        b2 = (np.asarray(dets, np.float64) ** 2).sum(1)
        a2 = np.array([(self.rows(k) ** 2).sum(1).max() for k in keys])
        return SAFETY * (2 * n + 3) * U * (a2[:, None] + b2[None, :])


def gate32(max_distance):
    return np.float32(max_distance) + np.float32(1e-5)


def assert_close_to_ref(got, ref, keys, dets, metric, n, max_distance=None, what=""):
    """Ungated: |got - ref| <= bound everywhere.  Gated: the same below the gate, exactly the gate value above it, nothing within
    GATE_BAND bounds of the gate.  Returns the largest error / bound ratio among the entries compared by value."""
    tol = ref.bound(keys, dets, metric, n)
    raw = ref.cost(keys, dets, metric)
    got = np.asarray(got)
    assert got.shape == raw.shape, (what, got.shape, raw.shape)
    if max_distance is None:
        err = np.abs(got.astype(np.float64) - raw)
        w = np.unravel_index(np.argmax(err / tol), err.shape)
        assert np.all(err <= tol), "%s: error %.3g against a bound of %.3g at %s" % (what, err[w], tol[w], w)
        return float((err / tol).max())
    below = raw < max_distance - GATE_BAND * tol
    above = raw > max_distance + GATE_BAND * tol
    err = np.abs(got.astype(np.float64) - raw)
    assert np.all(err[below] <= tol[below]), what
    assert np.all(got[above] == gate32(max_distance)), what
    return float((err[below] / tol[below]).max()) if below.any() else 0.0


# ----------------------------------------------------------------------------- the 16-lane butterfly of bank_cost96_kernel
def lane_detection(lane):
    """The detection lane `lane` of a 16-lane group ends with: j = 8 b0 + 4 b1 + 2 b2 + b3 (the lane's bits, reversed)."""
    lane = np.asarray(lane)
    return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3)


def butterfly_group(v, levels=(0, 1, 2, 3)):
    """numpy restatement of butterfly_group (csrc/bank96.hip; the first four levels of bank.hip's butterfly16).  v[lane][j]: lane's
    partial sum for detection j, 16 x 16.  At the step that uses lane bit s a lane keeps the upper half of its values when the bit is
    set (the lower half otherwise), and adds what its partner lane ^ (1 << s) sends: the half the partner does not keep.  `levels` is
    the order in which the lane bits are used (the kernel's: 0, 1, 2, 3).  Returns r[lane], one sum per lane."""
    cur = np.array(v, dtype=np.float64)
    assert cur.shape == (16, 16) and sorted(levels) == [0, 1, 2, 3]
    lanes = np.arange(16)
    for s in levels:
        half = cur.shape[1] // 2
        bit = ((lanes >> s) & 1).astype(bool)[:, None]
        keep = np.where(bit, cur[:, half:], cur[:, :half])
        send = np.where(bit, cur[:, :half], cur[:, half:])
        cur = keep + send[lanes ^ (1 << s)]
    return cur[:, 0]
