"""N x M distances on the device - mirrors of reid/losses/utils.py:12-35 and the brute-force k-NN of
reid/faiss_utils.py:56-139.  Inputs may be numpy arrays or torch tensors (CPU or GPU); outputs are numpy."""
import numpy as np

from . import _ffi
from .engine import Engine, get_engine


def _np(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _distmat(x, y, metric, device, precision):
    """precision None / "f32": today's call and bits; "f16x3": the dot product in the fp32-class arithmetic (reid_distmat_x3: |x| < 65504,
    |y| < 31.98, other bits, no rank promised); anything else is a ValueError before the device is touched."""
    Engine.distmat_precision_value(precision)
    return get_engine(device).distmat(_np(x), _np(y), metric, precision=precision)


def euclidean_dist(x, y, device=0, precision=None):
    """sqrt(clamp(|x|^2 + |y|^2 - 2 x.y^T, 1e-12)) - reid/losses/utils.py:21-35."""
    return _distmat(x, y, _ffi.METRIC_L2, device, precision)


def cosine_dist(x, y, device=0, precision=None):
    """(1 - cos)/2 - reid/losses/utils.py:12-18."""
    return _distmat(x, y, _ffi.METRIC_COS_HALF, device, precision)


def cosine_distance(x, y, device=0, precision=None):
    """1 - cos on L2-normalised rows: DeepSORT's appearance cost, gated by MAX_DIST 0.15 (deep_sort.yaml:3)."""
    return _distmat(x, y, _ffi.METRIC_COS, device, precision)


def nearest(x, y, metric=_ffi.METRIC_L2, device=0):
    """(argmin index int32[m], min value float32[m]) per row of the distance matrix; ties -> lowest index."""
    return get_engine(device).argmin_rows(_np(x), _np(y), metric)


def search_raw_array(xb, xq, k, device=0):
    """Brute-force squared-L2 k-NN, argument order of search_raw_array_pytorch(res, xb, xq, k)
    (reid/faiss_utils.py:56): returns (D float32[nq,k], I int32[nq,k])."""
    return get_engine(device).knn(_np(xq), _np(xb), k)


def nearest_x3(x, y, metric=_ffi.METRIC_L2, device=0):
    """`nearest` with the candidates from the fp32-class arithmetic on the f16 matrix pipe (reid_argmin_rows_x3): the same indices and
    values bit for bit, for finite operands with |x| < 65504 and |y| < 31.98 (outside: ReidHipError, status -3)."""
    return get_engine(device).argmin_rows(_np(x), _np(y), metric, precision="f16x3")


def search_raw_array_x3(xb, xq, k, device=0):
    """`search_raw_array` the same way (reid_knn_x3): the same (D, I) bit for bit, 1 <= k <= 24 (ValueError otherwise, before the device
    is touched), the domain of `nearest_x3`."""
    Engine.select_precision_entry("reid_knn", "f16x3", k)
    return get_engine(device).knn(_np(xq), _np(xb), k, precision="f16x3")


class IndexFlatL2:
    """The slice of faiss.IndexFlatL2 the reference uses (reid/faiss_utils.py:138-139,176-181): add + search."""

    def __init__(self, d, device=0):
        self.d, self.device = int(d), device
        self._xb = np.empty((0, self.d), np.float32)

    @property
    def ntotal(self):
        return self._xb.shape[0]

    def reset(self):
        self._xb = np.empty((0, self.d), np.float32)

    def add(self, x):
        x = _np(x)
        assert x.ndim == 2 and x.shape[1] == self.d
        self._xb = np.concatenate([self._xb, x], 0)

    def search(self, x, k):
        D, I = get_engine(self.device).knn(_np(x), self._xb, k)
        return D, I.astype(np.int64)
