"""ResNet18-IBN-SE at another input size: what the any-size forward costs.
    python tools/bench_anysize.py [--n 1024] [--repeats 5] [--out profiles/anysize_x3_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python3 tools/bench_anysize.py --trace [--forms _x3]    # one pass of each (or of the
                                                                                                 # forms named), for the per-kernel split
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Seed-0 weights with 751
classes, images resident on the device (64 distinct images tiled to n: the content does not change the work), the
embeddings and logits left there: device events around reid_embed_f32_nchw_hw_dev, so neither PCIe nor numpy is in the figure.  Prints (and
writes) one JSON line, every rate the mean over --repeats repeats with their standard deviation, minimum and maximum, one warm-up round
first, the repeats of the forms alternating:
  veri_224x268         images/s of n images at (224, 268), the evaluation script's VeRi geometry, through the any-size forward in exact fp32
                       (reid_ctx_set_hw_precision 0)
  veri_224x268_x3      the same in the fp32-class arithmetic (reid_ctx_set_hw_precision 2: any_conv_x3_kernel)
  generic_256x128      images/s of n images at (256, 128) through the any-size forward (debug switch anysize_force), exact fp32
  generic_256x128_x3   the same in the fp32-class arithmetic
  fixed_256x128        images/s of the same images through the existing mode-0 forward: generic / fixed is the cost of generality
  fixed_256x128_mode2  ... and through the existing mode-2 forward, the ceiling of the fp32-class forms
  pixels               the same as input megapixels/s
  x3_over_f32          per geometry: the ratio of the means, and `clear` = the fp32-class mean exceeds the exact-fp32 mean of the SAME call by
                       more than three of the larger standard deviation
Reported as measured: there is no threshold.  --trace runs one pass of each and nothing else (the kernel trace of that run, summed per
kernel by tools/rocprof_summary.py, is the per-kernel split quoted in DESIGN.md)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 1), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 1), "min": round(float(v.min()), 1),
            "max": round(float(v.max()), 1), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--forms", default="", help="with --trace: only the forms whose name ends with this (e.g. _x3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anysize_x3_bench.json"))
    args = ap.parse_args()
    from oracle import seres18
    from reid_amd import synth, weights
    from reid_amd.engine import any_pass_size, get_engine
    from reid_amd.parallel import DevArray

    n = args.n
    eng = get_engine(0)
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    d_emb, d_log = DevArray(eng, (n, 512), np.float32), DevArray(eng, (n, 751), np.float32)
    d_x = {}
    for h, w in ((224, 268), (256, 128)):
        base = seres18.preprocess_u8(synth.smooth_crops_u8(64, 3, h, w)).numpy()
        d_x[(h, w)] = DevArray.from_numpy(eng, np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1, 1, 1))[:n]))

    def run(size, force, hw_precision, mode):
        eng.debug_switch("anysize_force", int(force))
        eng.set_hw_precision(hw_precision)
        eng.set_precision(mode)
        try:
            eng.timer_start()
            eng.embed_f32_nchw_dev(d_x[size].ptr, n, d_emb.ptr, d_log.ptr, size=size)
            return eng.timer_stop()
        finally:
            eng.set_precision(0)
            eng.set_hw_precision(-1)
            eng.debug_switch("anysize_force", 0)

    # name: (size, anysize_force, reid_ctx_set_hw_precision, context mode)
    runs = {"veri_224x268": ((224, 268), False, 0, 0), "veri_224x268_x3": ((224, 268), False, 2, 0),
            "generic_256x128": ((256, 128), True, 0, 0), "generic_256x128_x3": ((256, 128), True, 2, 0),
            "fixed_256x128": ((256, 128), False, -1, 0), "fixed_256x128_mode2": ((256, 128), False, -1, 2)}
    ms = {k: [] for k in runs}
    if args.trace and args.forms:
        runs = {k: v for k, v in runs.items() if k.endswith(args.forms)}
    rounds = 1 if args.trace else args.repeats + 1
    for r in range(rounds):                      # round 0 warms up (workspaces, the side library, code objects)
        for name, form in runs.items():
            t = run(*form)
            if r > 0:
                ms[name].append(t)
    eng.sync()
    if args.trace:
        return
    out = {"workload": "anysize", "n": n, "num_class": 751, "unit": "images/s", "repeats": args.repeats,
           "pass_images": {"veri_224x268": any_pass_size(1024, 224, 268), "generic_256x128": 1024, "fixed_256x128": 1024}, "pixels": {}}
    out["precision"] = {name: ("f16x3" if form[2] == 2 or form[3] == 2 else "f32") for name, form in runs.items()}
    for name, (size, _, _, _) in runs.items():
        rate = n / (np.asarray(ms[name]) / 1e3)
        out[name] = stats(rate)
        out[name]["ms_per_call"] = stats(ms[name])
        out["pixels"][name] = round(float(rate.mean()) * size[0] * size[1] / 1e6, 1)
    out["generic_over_fixed"] = round(out["generic_256x128"]["mean"] / out["fixed_256x128"]["mean"], 4)
    out["generic_x3_over_fixed_mode2"] = round(out["generic_256x128_x3"]["mean"] / out["fixed_256x128_mode2"]["mean"], 4)
    out["x3_over_f32"] = {}
    for geom in ("veri_224x268", "generic_256x128"):
        a, b = out[geom], out[geom + "_x3"]
        out["x3_over_f32"][geom] = {"ratio": round(b["mean"] / a["mean"], 4), "clear": bool(b["mean"] - a["mean"] > 3 * max(a["std"], b["std"]))}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
