"""Swin flip-TTA descriptors: the new entry point against the same result from the calls that existed before it.
    python tools/bench_swin_eval.py [--n 1024] [--repeats 5] [--out profiles/swin_eval_bench.json]
One call, one box.  n images at 448 x 224 resident on the device (64 distinct synth.images_f32 images tiled to n: the content does not
change the work), Swin-T v1, seed-0 weights with 751 classes, fp32-class arithmetic (mode 2), one pass.  Prints (and writes) one JSON line:
  descriptor_dev     (a) descriptors/s of reid_swin_descriptor_f32_nchw_dev with flip_tta on, plus the download of the [n, 847] result
  embed_twice        (b) the same descriptors from existing calls: a host flip of the images (numpy) and its upload, two
                     reid_swin_embed_f32_nchw_dev with logits, the downloads, and the normalise / concatenate / average / renormalise in
                     numpy
  embed_twice_resident_flip   (b) without the host flip and its upload (the mirrored copy already on the device): what the two embed
                     calls, the downloads and numpy cost on their own
  max_abs_diff       largest difference between the results of (a) and (b) (the logits of (b) come from mode 2's GEMM, those of (a)
                     from exact fp32 on x_norm)
Each rate is the mean over --repeats repeats with their standard deviation, minimum and maximum; one warm-up round first; the repeats of
the three alternate.  Reported as measured: there is no threshold.  The mirrored stems save the 1.2 GB mirrored copy and one launch, not
time - the copy would be well under 1 % of a pass."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 448, 224


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 2), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 2), "min": round(float(v.min()), 2),
            "max": round(float(v.max()), 2), "n": int(len(v))}


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_eval_bench.json"))
    args = ap.parse_args()
    from reid_amd import synth, weights
    from reid_amd.engine import get_engine
    from reid_amd.parallel import DevArray

    n = args.n
    base = synth.images_f32(64, 5, h=H, w=W)
    x = np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1, 1, 1))[:n])
    eng = get_engine(0)
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    eng.set_precision(2)
    nc, dim = eng.swin_num_class, eng.swin_dim
    d_x, d_xf = DevArray(eng, x.shape, np.float32), DevArray(eng, x.shape, np.float32)
    d_out = DevArray(eng, (n, nc + dim), np.float32)
    d_e, d_l = [DevArray(eng, (n, dim), np.float32) for _ in range(2)], [DevArray(eng, (n, nc), np.float32) for _ in range(2)]
    eng.h2d(d_x.ptr, x)

    def new_entry():
        eng.swin_descriptor_dev(d_x.ptr, n, H, W, True, d_out.ptr)
        return d_out.numpy()

    def existing(resident_flip):
        if not resident_flip:
            eng.h2d(d_xf.ptr, np.ascontiguousarray(x[..., ::-1]))
        for v, src in enumerate((d_x, d_xf)):
            eng.swin_embed_dev(src.ptr, n, H, W, d_e[v].ptr, d_l[v].ptr)
        d = [np.concatenate([_unit(d_l[v].numpy()), _unit(d_e[v].numpy())], 1) for v in range(2)]
        return _unit((d[0] + d[1]) / 2.0)

    runs = {"descriptor_dev": new_entry, "embed_twice": lambda: existing(False), "embed_twice_resident_flip": lambda: existing(True)}
    rates = {k: [] for k in runs}
    results = {}
    for r in range(args.repeats + 1):            # round 0 warms up (workspaces, side libraries, the mirrored copy on the device)
        for name, fn in runs.items():
            eng.sync()
            t0 = time.perf_counter()
            results[name] = fn()
            eng.sync()
            if r:
                rates[name].append(n / (time.perf_counter() - t0))
    out = {"workload": "swin_eval", "n": n, "size": [H, W], "precision": 2, "version": "v1", "num_class": nc, "unit": "descriptors/s",
           "max_abs_diff": float(np.abs(results["descriptor_dev"] - results["embed_twice"]).max())}
    out.update({k: stats(v) for k, v in rates.items()})
    for a in [d_x, d_xf, d_out] + d_e + d_l:
        a.free()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
