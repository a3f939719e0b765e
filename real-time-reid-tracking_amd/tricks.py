"""The Market-1501 attribute distance of the evaluation script - mirror of reid/tricks/additional_market_attributes.py:11-38.

``get_attributes(file_name)`` reads the dataset's ``market_attribute.mat``; ``get_attribute_dist(labels, file_name)`` is the N x N matrix
the script adds to the Jaccard distances before DBSCAN (reid/image_reid_inference.py:276-289).  ``reid_inference.evaluate_reid(...,
attribute_dist=...)`` adds the same term on the device without materialising it (``reid_distmat_add_l2_dev``).
"""
import numpy as np

AGE_ONE_HOT = {1: [0, 0, 0, 1], 2: [0, 0, 1, 0], 3: [0, 1, 0, 0], 4: [1, 0, 0, 0]}   # :16
NUM_ATTRIBUTES = 30   # the age one-hot (4) + 26 attributes


def get_attributes(file_name):
    """{identity: int64 array [30]} of the FIRST field of the file's ``market_attribute`` struct, as the reference reads it (:12-14:
    ``loadmat(...)["market_attribute"][0][0][0][0][0]``): 27 attribute arrays - the first, age 1 .. 4, one-hot in reverse order - and the
    identities (``image_index``) last.  The struct's second field is not read, so its identities are unknown labels."""
    from scipy import io
    mat = io.loadmat(file_name)["market_attribute"][0][0]
    mat = mat[0][0][0]
    identities = [int(x.item()) for x in mat[-1][0]]
    out = {}
    for klass, identity in zip(range(len(mat[0][0])), identities):
        row = list(AGE_ONE_HOT[int(mat[0][0][klass])])
        row.extend(int(mat[i][0][klass]) for i in range(1, 27))
        out[identity] = np.asarray(row, np.int64)
    return out


def attribute_rows(labels, file_name):
    """float32 [N, 30]: the attribute row of every label in order; a label the table does not hold (0 and -1 included) gets ones (:33-35)."""
    table = get_attributes(file_name)
    ones = np.ones(NUM_ATTRIBUTES, np.float32)
    rows = [table[int(l)].astype(np.float32) if int(l) in table else ones for l in np.asarray(labels).reshape(-1)]
    return np.stack(rows) if rows else np.empty((0, NUM_ATTRIBUTES), np.float32)


def normalize_rows(rows):
    """F.normalize(rows, dim=1) in fp32: row / max(||row||, 1e-12) (:36)."""
    rows = np.ascontiguousarray(rows, np.float32)
    norm = np.sqrt((rows * rows).sum(1, dtype=np.float32, keepdims=True)).astype(np.float32)
    return (rows / np.maximum(norm, np.float32(1e-12))).astype(np.float32)


def get_attribute_dist(labels, file_name, device=0):
    """float32 [N, N] = euclidean_dist of the normalised attribute rows with themselves (:29-38), on the device."""
    from .distance import euclidean_dist
    rows = normalize_rows(attribute_rows(labels, file_name))
    return euclidean_dist(rows, rows, device=device)
