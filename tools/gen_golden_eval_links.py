#!/usr/bin/env python3
"""Fixtures of the evaluation chain's attribute distance (CPU only): python tools/gen_golden_eval_links.py --reference DIR

DIR is a checkout of the reference repository; its reid/tricks/additional_market_attributes.py is imported and run, none of its text
is copied.  Writes

  tests/golden/market_attribute_small.mat   a stand-in for Market-1501's market_attribute.mat with scipy.io.savemat: the struct
                                            ``market_attribute`` with two fields (train, test) of 12 and 11 identities, each a struct
                                            of 27 attribute arrays [1][K] (age 1 .. 4 first, the rest 1 / 2) plus ``image_index``, the
                                            identities as strings, last - the nesting the reference's get_attributes indexes
  tests/golden/eval_links.npz               the reference's own get_attributes table of that file (ids, table) and its
                                            get_attribute_dist for a label list with duplicates, 0, -1, an unknown id and an id of the
                                            second field (labels, dist)

Both files hold data only."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the attribute names of the dataset's file, in its order (age first, image_index last)
NAMES = ("age", "backpack", "bag", "handbag", "downblack", "downblue", "downbrown", "downgray", "downgreen", "downpink", "downpurple",
         "downwhite", "downyellow", "upblack", "upblue", "upgreen", "upgray", "uppurple", "upred", "upwhite", "upyellow", "clothes", "down",
         "up", "hair", "hat", "gender")
TRAIN_IDS = (2, 7, 10, 11, 12, 20, 22, 23, 27, 28, 30, 32)
TEST_IDS = (1, 3, 4, 5, 6, 8, 9, 13, 14, 15, 16)


def field(rng, ids):
    k = len(ids)
    cols = {"age": rng.integers(1, 5, (1, k)).astype(np.uint8)}
    for name in NAMES[1:]:
        cols[name] = rng.integers(1, 3, (1, k)).astype(np.uint8)
    # two identities with the same attributes: their distance is the clamp's value in the reference
    for name in NAMES:
        cols[name][0, 1] = cols[name][0, 0]
    idx = np.empty((1, k), object)
    for i, v in enumerate(ids):
        idx[0, i] = "%04d" % v
    cols["image_index"] = idx
    return cols


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    from scipy import io
    rng = np.random.default_rng(1501)
    train, test = field(rng, TRAIN_IDS), field(rng, TEST_IDS)
    dt = [(n, object) for n in NAMES + ("image_index",)]

    def struct(cols):
        s = np.empty((1, 1), dt)
        for n, _ in dt:
            s[n][0, 0] = cols[n]
        return s
    top = np.empty((1, 1), [("train", object), ("test", object)])
    top["train"][0, 0] = struct(train)
    top["test"][0, 0] = struct(test)
    mat_path = os.path.join(GOLDEN, "market_attribute_small.mat")
    io.savemat(mat_path, {"market_attribute": top})

    sys.path.insert(0, os.path.join(os.path.abspath(args.reference), "reid"))
    from tricks.additional_market_attributes import get_attribute_dist, get_attributes
    table = get_attributes(mat_path)
    ids = np.asarray(sorted(table), np.int64)
    assert tuple(ids) == tuple(sorted(TRAIN_IDS)), ids
    tab = np.stack([table[int(i)].numpy() for i in ids]).astype(np.int64)
    assert tab.shape == (len(TRAIN_IDS), 30)
    # duplicates, the two identical identities (2 and 7), 0, -1, an unknown id (999) and an id of the second field (3)
    labels = [2, 7, 2, 10, 0, -1, 999, 3, 11, 12, 20, 20, 22, 23, 27, 28, 30, 32, 7, 10]
    dist = get_attribute_dist(labels, mat_path)
    assert dist.dtype == np.float32 and dist.shape == (len(labels), len(labels))
    np.savez_compressed(os.path.join(GOLDEN, "eval_links.npz"), ids=ids, table=tab, labels=np.asarray(labels, np.int64), dist=dist)
    print("wrote", mat_path, os.path.getsize(mat_path), "bytes; table", tab.shape, "dist", dist.shape, "diag", np.unique(np.diag(dist)))


if __name__ == "__main__":
    main()
