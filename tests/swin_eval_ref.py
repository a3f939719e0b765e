"""float64 restatement of swin_descriptor_kernel (csrc/swin_eval.hip) with a bound per element, shared by tests/test_swin_eval_host.py
and tests/test_gpu_swin_eval.py.

The descriptor of the evaluation script for a Swin (reid/image_reid_inference.py:112-123,252-253; swin_transformer.py:422-423 returns
(logits, x_norm)):   d(e) = [normalize(W e) | normalize(e)],   one view: d(e1);   two: normalize((d(e1) + d(e2)) / 2),
normalize = F.normalize, v / max(||v||, 1e-12).

The bound follows the kernel's arithmetic, not observed numbers.  u = 2^-24, g_n = n u / (1 - n u) (Higham 3.1).
  logits     l_k = sum_j w_kj e_j, K = 96 terms in one FMA chain s_j = fl(s_(j-1) + w_kj e_j): each step rounds once, relative to the
             partial sum it produces, so   |dl_k| <= u sum_j |s_j|   (running error bound, Higham 3.3; the s_j are taken from the
             float64 chain in the kernel's order, j = 0 .. 95).  The a-priori form g_96 sum_j |w_kj e_j| is ten times wider here and
             would put the norm's error above one hundredth of the fixture's TTA effect.
  norms      s = sum of squares, every product and addition one rounding; a thread adds ceil(len / 256) squares in order, six shuffle
             levels and two LDS levels follow: depth D = ceil(len / 256) + 9, so s carries a relative g_D; the square root halves it and
             adds its own rounding (<= 2u), and the computed vector differs from the true one: | ||l^|| - ||l|| | <= ||dl||.
             rel(norm) = ||dl|| / ||l|| + g_D / 2 + 2u    (x_norm is an input: dl = 0, len = 96).
  division   v_k = l_k / norm, <= 2u:     |dv_k| <= |dl_k| / ||l|| + |v_k| (rel(norm) + 2u).
  average    m_k = (v_k + w_k) / 2: one rounding, the halving is exact:     |dm_k| <= (|dv_k| + |dw_k|) / 2 + u |m_k|.
  last norm  as above with len = num_class + 96:   |do_k| <= |dm_k| / ||m|| + |o_k| (||dm|| / ||m|| + g_D' / 2 + 4u).
Everything is multiplied by SAFETY = 2 for the second-order terms dropped (the factor of the other kernel-level modules).  A zero row
has zero error and a zero bound: every term is proportional to a magnitude of the row.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
DIM = 96
EPS = 1e-12


def gamma(n):
    return n * U / (1.0 - n * U)


def _depth(length):
    return -(-length // 256) + 9


def _view(e, w):
    """d(e) [n, nc + 96] and its bound, before SAFETY."""
    e, w = np.asarray(e, np.float64), np.asarray(w, np.float64)
    lg = e @ w.T
    dl = U * np.abs(np.cumsum(e[:, None, :] * w[None, :, :], axis=2)).sum(2)       # u sum_j |s_j|, s_j the partial sums in k order
    nl = np.maximum(np.linalg.norm(lg, axis=1, keepdims=True), EPS)
    ne = np.maximum(np.linalg.norm(e, axis=1, keepdims=True), EPS)
    vl, ve = lg / nl, e / ne
    rel_l = np.linalg.norm(dl, axis=1, keepdims=True) / nl + gamma(_depth(w.shape[0])) / 2 + 2 * U
    rel_e = gamma(_depth(DIM)) / 2 + 2 * U
    return np.concatenate([vl, ve], 1), np.concatenate([dl / nl + np.abs(vl) * (rel_l + 2 * U), np.abs(ve) * (rel_e + 2 * U)], 1)


def descriptor64(e1, e2, cls_w):
    """(descriptor float64 [n, num_class + 96], bound of the same shape) for x_norm e1 (and e2, or None) [n, 96], cls_w [num_class, 96]."""
    d1, b1 = _view(e1, cls_w)
    if e2 is None:
        return d1, SAFETY * b1
    d2, b2 = _view(e2, cls_w)
    m = (d1 + d2) / 2.0
    dm = (b1 + b2) / 2.0 + U * np.abs(m)
    nm = np.maximum(np.linalg.norm(m, axis=1, keepdims=True), EPS)
    o = m / nm
    rel = np.linalg.norm(dm, axis=1, keepdims=True) / nm + gamma(_depth(m.shape[1])) / 2 + 4 * U
    return o, SAFETY * (dm / nm + np.abs(o) * rel)


def descriptor_from_parts(lg1, xn1, lg2=None, xn2=None):
    """The same rule from given logits (float64): the fixture's blocks -> the fixture's descriptors."""
    def nrm(v):
        v = np.asarray(v, np.float64)
        return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), EPS)
    d1 = np.concatenate([nrm(lg1), nrm(xn1)], 1)
    if lg2 is None:
        return d1
    return nrm((d1 + np.concatenate([nrm(lg2), nrm(xn2)], 1)) / 2.0)
