"""Arg-min and k-NN: the exact entries (reid_argmin_rows_dev, reid_knn_dev) beside the entries with fp32-class candidates
(reid_argmin_rows_x3_dev, reid_knn_x3_dev; csrc/select_x3.hip) - the same answers bit for bit, so only the time differs.
    python tools/bench_select_x3.py [--repeats 5] [--iters 50] [--out profiles/select_x3_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python3 tools/bench_select_x3.py --trace      # one call of each entry per shape: the
                                                                                                    # kernels' own times (tools/rocprof_summary.py)
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Operands resident on the
device (unit-length rows, random or - the last three cases - a gallery sorted by identity; inside the new entries' domain), the answers left there: device events around --iters back-to-back
calls of one entry; the row norms, the padded copy of the 1263-wide shape, every launch of the pipeline and the launch gaps are in the
figure.  One warm-up round, then --repeats rounds with the two entries alternating.  Prints (and writes) one JSON line; per case
  f32 / f16x3     ms per call: mean, standard deviation, minimum and maximum over the repeats
  x3_over_f32     time ratio f16x3 / f32 of the means (below 1: the new entry is faster), `clear` = the means differ by more than three
                  of the larger standard deviation
  f32_path        what the exact entry runs at the shape: the fused fp32 kernels of dist_select.hip, or knn_wide.hip (the k = 20 cases)
  recomputed      rows the new entry sent through the exact-row kernel (reid_debug_select_x3), of m - it depends on the ORDER of the
                  gallery: the sorted cases are there to show the cost of that
  equal           the two entries' answers compared bit for bit
Reported as measured: there is no threshold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (m, n, d, k): k = 0 is the arg-min (metric L2, the evaluation's).  Market-1501's query x gallery shard, the headline's 4096^2, and the
# re-ranking's all-pairs search at the descriptor width; at both k = 20 shapes reid_knn_dev takes knn_wide
# per_id > 0: a gallery SORTED BY IDENTITY instead of random rows - per_id consecutive images of each identity (a unit centre + 0.25 of a
# unit noise vector), one further image of an identity per query: a query's near columns are neighbours, tile lists overflow and their
# rows go to the exact-row kernel (21 = Market-1501's mean images per gallery identity; 48 = more than a tile list holds)
CASES = ((3368, 15913, 512, 0, 0), (4096, 4096, 512, 0, 0), (3368, 15913, 512, 20, 0), (19281, 19281, 1263, 20, 0),
         (3368, 15913, 512, 0, 21), (3368, 15913, 512, 20, 21), (3368, 15913, 512, 0, 48))


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 4), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 4), "min": round(float(v.min()), 4),
            "max": round(float(v.max()), 4), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_x3_bench.json"))
    args = ap.parse_args()
    from reid_amd import _ffi
    from reid_amd.engine import get_engine
    from reid_amd.parallel import DevArray

    eng = get_engine(0)
    out = {"workload": "select_x3", "unit": "ms per call", "repeats": args.repeats, "iters": args.iters, "cases": {}}
    for m, n, d, k, per_id in CASES:
        rng = np.random.default_rng(m + n + d + k + per_id)
        def unit(a):
            return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
        if per_id:
            centres = unit(rng.normal(size=((n + per_id - 1) // per_id, d)))
            y = unit(centres[np.arange(n) // per_id] + 0.25 * unit(rng.normal(size=(n, d))))
            x = unit(centres[rng.integers(0, len(centres), m)] + 0.25 * unit(rng.normal(size=(m, d))))
        else:
            x = unit(rng.normal(size=(m, d)))
            y = x if k and m == n else unit(rng.normal(size=(n, d)))      # the re-ranking searches a set against itself
        kk = max(k, 1)
        dx, dy = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y)
        dD, dI = DevArray(eng, (m, kk)), DevArray(eng, (m, kk), np.int32)
        iters = 1 if args.trace else args.iters

        def call(precision):
            if k:
                eng.knn_dev(dx.ptr, m, dy.ptr, n, d, k, dD.ptr, dI.ptr, precision=precision)
            else:
                eng.argmin_rows_dev(dx.ptr, m, dy.ptr, n, d, _ffi.METRIC_L2, dI.ptr, dD.ptr, precision=precision)

        def run(precision):
            eng.timer_start()
            for _ in range(iters):
                call(precision)
            return eng.timer_stop() / iters

        try:
            ms = {"f32": [], "f16x3": []}
            for r in range(1 if args.trace else args.repeats + 1):      # round 0 warms up (workspaces, the side library, code objects)
                for p in ms:
                    t = run(p)
                    if r > 0:
                        ms[p].append(t)
            eng.sync()
            if args.trace:
                continue
            got = {}
            for p in ms:
                call(p)
                eng.sync()
                got[p] = (dD.numpy().view(np.uint32), dI.numpy())
            st = eng.debug_select_x3(dx.ptr, m, dy.ptr, n, d, _ffi.METRIC_L2SQR if k else _ffi.METRIC_L2, kk, dD.ptr, dI.ptr)
            a, b = stats(ms["f32"]), stats(ms["f16x3"])
            out["cases"]["%s %dx%dx%d%s" % ("k=%d" % k if k else "argmin", m, n, d, " sorted by identity, %d each" % per_id if per_id else "")] = {
                "f32": a, "f16x3": b, "iters": iters,
                "x3_over_f32": {"ratio": round(b["mean"] / a["mean"], 4), "clear": bool(abs(b["mean"] - a["mean"]) > 3 * max(a["std"], b["std"]))},
                "f32_path": "knn_wide" if k else "fused fp32 (dist_select)", "recomputed": st["recomputed"], "rows": m,
                "recomputed_share": round(st["recomputed"] / m, 4),
                "equal": bool(np.array_equal(got["f32"][0], got["f16x3"][0]) and np.array_equal(got["f32"][1], got["f16x3"][1]))}
        finally:
            for arr in (dx, dy, dD, dI):
                arr.free()
    if args.trace:
        return
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
