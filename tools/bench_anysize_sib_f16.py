"""CARes18-IBN and EMARes18-IBN at another input size in fp16 storage (reid_ctx_set_hw_sib_f16 1, libreid_hip_anysize_sib_f16.so) against
the arithmetics they had there before, and against seres18_ibn in fp16 storage.
    python tools/bench_anysize_sib_f16.py [--repeats 5] [--no-trace] [--out profiles/anysize_sib_f16_bench.json]
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Seed-0 weights with 751
classes.  Prints (and writes) one JSON line; every figure is the mean over --repeats repeats with their standard deviation, minimum and
maximum, after one warm-up round, the forms alternating inside each repeat:
  passes    per sibling: images/s of n images resident on the device (64 distinct images tiled to n) through reid_embed_f32_nchw_hw_dev,
            embeddings and logits left there, between two device events (reid_timer_*): (128, 64) and (224, 268), n = 30 and n = 1024, in
            four forms - `hw_sib_f16` (the new setting), `hw_precision_2` and `hw_precision_0` (the same sibling with hw_siblings / hw_ema
            1, fp32-class and exact fp32) and `seres18_hw_f16` (seres18_ibn weights with hw_f16 1, loaded for that window; loading is
            outside the events).  A window holds LAUNCHES[n] calls.  `sib_f16_over_x3`: the ratio of the means and `slower` = the
            hw_sib_f16 mean is below the hw_precision-2 mean of the same call.
  kernels   per sibling and size: the share of the block tail's kernels (any_sib_*) and of every kernel in one pass of 1024 images with
            hw_sib_f16 1, from the device timestamps of a `rocprofv3 --kernel-trace --stats` run of --child trace (a fresh process,
            started before this one touches the device, no counters; every other figure is taken afterwards with the profiler off)
Reported as measured: there is no threshold."""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_anysize_f16 import LAUNCHES, NS, SIZES, device_images, short, timed  # noqa: E402
from bench_tracking_hw import seres_weights  # noqa: E402
from bench_tracking_swin import dispatches, stats  # noqa: E402

SIBS = ("cares18_ibn", "emares18_ibn")
FORMS = ("hw_sib_f16", "hw_precision_2", "hw_precision_0", "seres18_hw_f16")


def sibling_weights(arch):
    from reid_amd import synth, weights
    make = synth.cares18_state_dict if arch == "cares18_ibn" else synth.emares18_state_dict
    return weights.pack_seres18(make(0))[:2]


def engine():
    from reid_amd.engine import get_engine
    eng = get_engine(0)
    eng.set_precision(0)
    return eng


def child_trace():
    """Per sibling and size: 1024 images with hw_sib_f16 1 twice - the first call warms up, the second is the one kernel_shares keeps."""
    from reid_amd.parallel import DevArray
    eng = engine()
    d_emb, d_log = DevArray(eng, (1024, 512), np.float32), DevArray(eng, (1024, 751), np.float32)
    for arch in SIBS:
        eng.load_seres18(*sibling_weights(arch))
        eng.set_hw_sib_f16(True)
        for size in SIZES:
            d_x = device_images(eng, size, 1024)
            for _ in range(2):
                eng.embed_f32_nchw_dev(d_x.ptr, 1024, d_emb.ptr, d_log.ptr, size=size)
                eng.sync()
            d_x.free()
        eng.set_hw_sib_f16(False)
    eng.sync()


def kernel_shares(rows):
    """The trace in start order -> per sibling and size {tail_share, kernel_us_per_1024, share per kernel}; of the two traced calls of a
    (sibling, size) the second is kept."""
    passes, cur = [], None
    for name, st, en in rows:
        n = short(name)
        if "any_nchw_to_nhwc3_kernel" in n:       # every pass opens with the layout kernel (se_any_run_nchw)
            cur = collections.OrderedDict()
            passes.append(cur)
        if cur is not None:
            cur[n] = cur.get(n, 0.0) + (en - st) / 1e3
    counts = {SIZES[0]: 1, SIZES[1]: 2}            # 1024 images: one pass at (128, 64) (pass size 4096), two at (224, 268) (545)
    out, i = {}, 0
    for arch in SIBS:
        out[arch] = {}
        for size in SIZES:
            i += counts[size]                      # the warm-up
            tot = collections.OrderedDict()
            for p in passes[i:i + counts[size]]:
                for k, v in p.items():
                    tot[k] = tot.get(k, 0.0) + v
            i += counts[size]
            total = sum(tot.values())
            out[arch]["%dx%d" % size] = {"kernel_us_per_1024": round(total, 1),
                                         "tail_share": round(sum(v for k, v in tot.items() if "any_sib_" in k) / total, 4),
                                         "share": {k: round(v / total, 4) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])}}
    if i != len(passes):
        raise RuntimeError("%d passes in the trace, expected %d" % (len(passes), i))
    return out


def trace_child(keep_dir):
    d = os.path.join(keep_dir, "trace_sib_f16")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", "trace"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return dispatches(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anysize_sib_f16_bench.json"))
    ap.add_argument("--child", choices=["trace"], default=None)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernels is then reported as not taken)")
    args = ap.parse_args()
    if args.child == "trace":
        return child_trace()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (every figure comes with its spread)")

    out = {"workload": "anysize_sib_f16: cares18_ibn / emares18_ibn / seres18_ibn seed 0, 751 classes, device-resident images, device events "
                       "around reid_embed_f32_nchw_hw_dev; %d repeats, forms alternating inside a repeat" % args.repeats, "unit": "images/s"}
    if args.no_trace:
        out["kernels"] = "not taken (--no-trace)"
    else:
        with tempfile.TemporaryDirectory() as tmp:          # the trace first: this process has not opened the device yet
            try:
                out["kernels"] = kernel_shares(trace_child(tmp))
            except (RuntimeError, subprocess.TimeoutExpired, OSError) as e:   # said in the result, never papered over
                out["kernels"] = "not taken: the trace run failed: %s" % (str(e)[-400:],)

    from reid_amd.parallel import DevArray
    eng = engine()
    d_emb, d_log = DevArray(eng, (1024, 512), np.float32), DevArray(eng, (1024, 751), np.float32)
    blobs = {arch: sibling_weights(arch) for arch in SIBS}
    blobs["seres18_ibn"] = seres_weights()
    loaded = [None]

    def run(arch, form, d_x, n, size):
        want = "seres18_ibn" if form == "seres18_hw_f16" else arch
        if loaded[0] != want:                               # outside the timed window
            eng.load_seres18(*blobs[want])
            loaded[0] = want
        eng.set_hw_sib_f16(form == "hw_sib_f16")
        eng.set_hw_f16(form == "seres18_hw_f16")
        eng.set_hw_siblings(form.startswith("hw_precision") and arch == "cares18_ibn")
        eng.set_hw_ema(form.startswith("hw_precision") and arch == "emares18_ibn")
        eng.set_hw_precision({"hw_precision_2": 2, "hw_precision_0": 0}.get(form, -1))
        try:
            return timed(eng, d_x, n, size, d_emb, d_log, LAUNCHES[n])
        finally:
            eng.set_hw_sib_f16(False)
            eng.set_hw_f16(False)
            eng.set_hw_siblings(False)
            eng.set_hw_ema(False)
            eng.set_hw_precision(-1)

    out["passes"], out["sib_f16_over_x3"] = {}, {}
    for arch in SIBS:
        out["passes"][arch], out["sib_f16_over_x3"][arch] = {}, {}
        for size in SIZES:
            for n in NS:
                d_x = device_images(eng, size, n)
                ms = {k: [] for k in FORMS}
                for r in range(args.repeats + 1):            # round 0 warms up (workspaces, side libraries, code objects)
                    for form in FORMS:
                        t = run(arch, form, d_x, n, size)
                        if r > 0:
                            ms[form].append(t)
                d_x.free()
                key = "%dx%d n=%d" % (size[0], size[1], n)
                res = {form: dict(stats(n / (np.asarray(v) / 1e3)), ms_per_call=stats(v), calls_per_window=LAUNCHES[n]) for form, v in ms.items()}
                out["passes"][arch][key] = res
                a, b = res["hw_sib_f16"], res["hw_precision_2"]
                out["sib_f16_over_x3"][arch][key] = {"ratio": round(a["mean"] / b["mean"], 4), "slower": bool(a["mean"] < b["mean"]),
                                                     "clear": bool(abs(a["mean"] - b["mean"]) > 3 * max(a["std"], b["std"]))}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
