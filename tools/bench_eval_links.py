"""The evaluation chain's two links beside what they replace.
    python tools/bench_eval_links.py [--repeats 5] [--out profiles/eval_links_bench.json]

One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  One warm-up round, then
--repeats rounds with the two sides alternating; every figure is mean +- standard deviation (ddof 1) over the repeats, in ms.
  descriptors  1024 Market-size (128 x 64) uint8 images, host in -> host out, wall clock around one call: descriptor_images_u8_shift
               (the shifted mirrored view, random offsets, pad 10) against descriptor_images_u8(flip_tta=True) (the plain mirror);
               synthetic seres18_ibn weights, exact fp32
  add          N = 19 281 (Market's gallery + query), 30-wide normalised attribute rows, everything resident on the device, wall clock
               around --iters back-to-back rounds and a synchronisation: reid_distmat_add_l2_dev in place (one read and one write of the
               N x N matrix) against reid_distmat_dev into a second N x N buffer plus a separate in-place add of the two (torch's add_ on
               the same memory; the synchronisation between the two libraries' streams is inside the figure, some tens of microseconds)
Prints (and writes) one JSON line.  Reported as measured: there is no threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 4), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 4), "n": int(len(v))}


def ratio(new, old):
    return {"ratio": round(new["mean"] / old["mean"], 4), "clear": bool(abs(new["mean"] - old["mean"]) > 3 * max(new["std"], old["std"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--n", type=int, default=19281)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_links_bench.json"))
    args = ap.parse_args()
    import torch
    from reid_amd import _ffi, synth, weights
    from reid_amd.engine import get_engine

    eng = get_engine(0)
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    out = {"workload": "eval_links", "unit": "ms", "repeats": args.repeats}

    rng = np.random.default_rng(0)
    images = list(synth.smooth_crops_u8(args.images, 1, 128, 64))
    tl = rng.integers(0, 21, (args.images, 2)).astype(np.int32)
    sides = {"shift": lambda: eng.descriptor_images_u8_shift(images, tl, pad=10), "flip": lambda: eng.descriptor_images_u8(images, flip_tta=True)}
    ms = {k: [] for k in sides}
    for r in range(args.repeats + 1):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            fn()
            if r > 0:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    a, b = stats(ms["shift"]), stats(ms["flip"])
    out["descriptors"] = {"images": args.images, "source": "128x64 uint8", "descriptor_images_u8_shift": a, "descriptor_images_u8_flip": b,
                          "shift_over_flip": ratio(a, b)}

    n, d = args.n, 30
    rows = rng.integers(1, 3, (n, d)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    dev = torch.device("cuda:0")
    t_a = torch.from_numpy(rows).to(dev)
    t_j = torch.rand((n, n), device=dev, dtype=torch.float32)
    t_tmp = torch.empty((n, n), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()

    def fused():
        for _ in range(args.iters):
            eng.distmat_add_l2_dev(t_a.data_ptr(), n, d, t_j.data_ptr())
        eng.sync()

    def separate():
        for _ in range(args.iters):
            eng.distmat_dev(t_a.data_ptr(), n, t_a.data_ptr(), n, d, _ffi.METRIC_L2, t_tmp.data_ptr())
            eng.sync()
            t_j.add_(t_tmp)
            torch.cuda.synchronize()

    sides = {"fused": fused, "separate": separate}
    ms = {k: [] for k in sides}
    for r in range(args.repeats + 1):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            fn()
            if r > 0:
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.iters)
    a, b = stats(ms["fused"]), stats(ms["separate"])
    a["gbs"] = round(8.0 * n * n / (a["mean"] * 1e-3) / 1e9, 1)          # one read and one write of the matrix
    out["add"] = {"n": n, "d": d, "iters": args.iters, "reid_distmat_add_l2_dev": a, "reid_distmat_dev_plus_add": b, "fused_over_separate": ratio(a, b)}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
