"""The N x M distance matrix: the exact entry (reid_distmat_dev, fp32 MFMA) beside the fp32-class one (reid_distmat_x3_dev, dist_x3_kernel).
    python tools/bench_distmat_x3.py [--repeats 5] [--iters 50] [--out profiles/distmat_x3_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python3 tools/bench_distmat_x3.py --trace     # one call of each entry per shape: the
                                                                                                    # kernels' own times (tools/rocprof_summary.py)
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Operands resident on the
device (unit-length random rows: the content does not change the work, and lies inside the new entry's domain), the matrix left there:
device events around --iters back-to-back calls of one entry, so neither PCIe nor numpy is in the figure; the row norms, the padded copy
of the 1263-wide shape and the launch gaps are (they are part of the call).  One warm-up round, then --repeats rounds with the two entries
alternating.  Prints (and writes) one JSON line; per shape m x n x d (metric L2, the evaluation's):
  f32 / f16x3     ms per call: mean, standard deviation, minimum and maximum over the repeats; tflops = 2 m n d / mean
  x3_over_f32     time ratio f16x3 / f32 of the means (below 1: the new entry is faster), and `clear` = the means differ by more than three
                  of the larger standard deviation
  max_abs_diff    the largest difference between the two matrices (a sanity figure, the bounds are the tests')
Reported as measured: there is no threshold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Market-1501's query x gallery shard at the embedding width, the headline's 4096^2, the re-ranking's N at the descriptor width
SHAPES = ((3368, 15913, 512), (4096, 4096, 512), (4096, 19281, 1263))


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 4), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 4), "min": round(float(v.min()), 4),
            "max": round(float(v.max()), 4), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distmat_x3_bench.json"))
    args = ap.parse_args()
    from reid_amd import _ffi
    from reid_amd.engine import get_engine
    from reid_amd.parallel import DevArray

    eng = get_engine(0)
    metric = _ffi.METRIC_L2
    out = {"workload": "distmat_x3", "metric": "L2", "unit": "ms per call", "repeats": args.repeats, "iters": args.iters, "shapes": {}}
    for m, n, d in SHAPES:
        rng = np.random.default_rng(m + n + d)
        x = rng.normal(size=(m, d)).astype(np.float32)
        y = rng.normal(size=(n, d)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        y /= np.linalg.norm(y, axis=1, keepdims=True)
        dx, dy, do = DevArray.from_numpy(eng, x), DevArray.from_numpy(eng, y), DevArray(eng, (m, n))

        def run(precision, iters):
            eng.timer_start()
            for _ in range(iters):
                eng.distmat_dev(dx.ptr, m, dy.ptr, n, d, metric, do.ptr, precision=precision)
            return eng.timer_stop() / iters

        try:
            ms = {"f32": [], "f16x3": []}
            rounds = 1 if args.trace else args.repeats + 1
            for r in range(rounds):                  # round 0 warms up (workspaces, the side library, code objects)
                for p in ms:
                    t = run(p, 1 if args.trace else args.iters)
                    if r > 0:
                        ms[p].append(t)
            eng.sync()
            if args.trace:
                continue
            got = {}
            for p in ms:
                eng.distmat_dev(dx.ptr, m, dy.ptr, n, d, metric, do.ptr, precision=p)
                eng.sync()
                got[p] = do.numpy()
            a, b = stats(ms["f32"]), stats(ms["f16x3"])
            for s in (a, b):
                s["tflops"] = round(2.0 * m * n * d / (s["mean"] * 1e-3) / 1e12, 1)
            out["shapes"]["%dx%dx%d" % (m, n, d)] = {
                "f32": a, "f16x3": b,
                "x3_over_f32": {"ratio": round(b["mean"] / a["mean"], 4), "clear": bool(abs(b["mean"] - a["mean"]) > 3 * max(a["std"], b["std"]))},
                "max_abs_diff": float(np.abs(got["f32"] - got["f16x3"]).max())}
        finally:
            for arr in (dx, dy, do):
                arr.free()
    if args.trace:
        return
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
