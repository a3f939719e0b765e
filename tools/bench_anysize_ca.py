"""CARes18-IBN at another input size: what the TripletAttention tail of libreid_hip_anysize_ca.so costs, against the kernels of the
256 x 128 forward (csrc/attention_f32.hip) in the same trunk and against seres18_ibn through the same entry.
    python tools/bench_anysize_ca.py [--repeats 5] [--out profiles/anysize_ca_bench.json]
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Seed-0 weights with 751
classes, images resident on the device (64 distinct images tiled to n: the content does not change the work), embeddings and logits
left there: device events around reid_embed_f32_nchw_hw_dev, so neither PCIe nor numpy is in the figure.  Prints (and writes) one JSON line;
every rate is the mean over --repeats repeats with their standard deviation, minimum and maximum, one warm-up round first, the repeats of
the forms alternating.  Per size (224 x 268, the script's VeRi geometry; 128 x 64, a DeepSORT crop), pass (1024 and 30 images) and
reid_ctx_set_hw_precision (0 exact fp32, 2 fp32-class):
  ca_new    images/s of cares18_ibn, reid_ctx_set_hw_siblings 1, debug switch any_ca 1 (the new library)
  ca_old    the same with any_ca 0 (ta_stats_kernel / ta_gate_kernel / ta_apply_kernel in the any-size trunk)
  se        seres18_ibn through the same entry: the reference point
  new_over_old   the ratio of the means, and `clear` = the means differ by more than three of the larger standard deviation
Reported as measured: there is no threshold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((224, 268), (128, 64))
PASSES = (1024, 30)


def stats(v, digits=1):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), digits), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, digits),
            "min": round(float(v.min()), digits), "max": round(float(v.max()), digits), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anysize_ca_bench.json"))
    args = ap.parse_args()
    from oracle import seres18
    from reid_amd import synth, weights
    from reid_amd.engine import any_pass_size, get_engine
    from reid_amd.parallel import DevArray

    eng = get_engine(0)
    eng.set_precision(0)
    blobs = {"se": weights.pack_seres18(synth.seres18_state_dict(0))[:2], "ca": weights.pack_seres18(synth.cares18_state_dict(0))[:2]}
    nmax = max(PASSES)
    d_emb, d_log = DevArray(eng, (nmax, 512), np.float32), DevArray(eng, (nmax, 751), np.float32)
    d_x = {}
    for h, w in SIZES:
        base = seres18.preprocess_u8(synth.smooth_crops_u8(64, 3, h, w)).numpy()
        d_x[(h, w)] = DevArray.from_numpy(eng, np.ascontiguousarray(np.tile(base, ((nmax + 63) // 64, 1, 1, 1))[:nmax]))

    def run(size, n, hw_precision, any_ca):
        eng.debug_switch("any_ca", any_ca)
        eng.set_hw_precision(hw_precision)
        try:
            eng.timer_start()
            eng.embed_f32_nchw_dev(d_x[size].ptr, n, d_emb.ptr, d_log.ptr, size=size)
            return eng.timer_stop()
        finally:
            eng.set_hw_precision(-1)
            eng.debug_switch("any_ca", 1)

    forms = [(size, n, p) for size in SIZES for n in PASSES for p in (0, 2)]
    ms = {(f, which): [] for f in forms for which in ("ca_new", "ca_old", "se")}
    try:
        for r in range(args.repeats + 1):            # round 0 warms up (workspaces, the side libraries, code objects)
            for arch in ("ca", "se"):                # one load per architecture and round
                eng.load_seres18(*blobs[arch])
                eng.set_hw_siblings(arch == "ca")
                for f in forms:
                    for which, any_ca in ((("ca_new", 1), ("ca_old", 0)) if arch == "ca" else (("se", 1),)):
                        t = run(f[0], f[1], f[2], any_ca)
                        if r > 0:
                            ms[(f, which)].append(t)
        eng.sync()
    finally:
        eng.set_hw_siblings(False)
    out = {"workload": "anysize_ca", "num_class": 751, "unit": "images/s", "repeats": args.repeats, "results": []}
    for size, n, p in forms:
        row = {"size": list(size), "n": n, "hw_precision": p, "pass_images": min(n, any_pass_size(1024, *size))}
        for which in ("ca_new", "ca_old", "se"):
            t = np.asarray(ms[((size, n, p), which)])
            row[which] = stats(n / (t / 1e3))
            row[which]["ms_per_call"] = stats(t, 3)
        a, b = row["ca_new"], row["ca_old"]
        row["new_over_old"] = {"ratio": round(a["mean"] / b["mean"], 4), "clear": bool(abs(a["mean"] - b["mean"]) > 3 * max(a["std"], b["std"]))}
        row["ca_new_over_se"] = round(a["mean"] / row["se"]["mean"], 4)
        out["results"].append(row)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
