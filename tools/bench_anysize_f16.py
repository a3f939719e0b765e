"""ResNet18-IBN-SE at another input size in fp16 storage (reid_ctx_set_hw_f16 1, libreid_hip_anysize_f16.so) against the arithmetic it
had there before.
    python tools/bench_anysize_f16.py [--repeats 5] [--frames 300] [--no-trace] [--out profiles/anysize_f16_bench.json]
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  seres18_ibn seed-0 weights
with 751 classes.  Prints (and writes) one JSON line; every figure is the mean over --repeats repeats with their standard deviation,
minimum and maximum, after one warm-up round, the forms alternating inside each repeat:
  passes    images/s of n images resident on the device (64 distinct images tiled to n) through reid_embed_f32_nchw_hw_dev, embeddings and
            logits left there, between two device events (reid_timer_*): (128, 64) and (224, 268), n = 30 and n = 1024, with hw_f16 1,
            with hw_precision 2 (fp32-class) and with hw_precision 0 (exact fp32).  A window holds LAUNCHES[n] calls, so that the 30-image
            windows are not a fraction of a millisecond.  `f16_over_x3`: the ratio of the means and `slower` = the hw_f16 mean is below
            the hw_precision-2 mean of the same call.
  generic   (256, 128) x 1024 through the new forward (debug switch anysize_force, hw_f16 1) against the fixed-size mode-1 forward
  stream    frames/s of tracking.CameraStream(arch="seres18_hw", size=(128, 64)) with hw_f16=True against hw_precision="f16x3", the stream
            stand-in and the method of tools/bench_tracking_hw.py (two contexts, the repeats of the two alternating)
  kernels   the share of each kernel in one pass of 1024 images at either size with hw_f16 1, from the device timestamps of a
            `rocprofv3 --kernel-trace --stats` run of --child trace (a fresh process, started before this one touches the device, no
            counters; every other figure is taken afterwards with the profiler off)
Reported as measured: there is no threshold."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tracking_hw import Standin, run_stream, seres_weights  # noqa: E402
from bench_tracking_swin import BUDGET, MAX_DIST, dispatches, stats  # noqa: E402

SIZES = ((128, 64), (224, 268))
NS = (30, 1024)
LAUNCHES = {30: 20, 1024: 2}
FORMS = {"hw_f16": (True, -1), "hw_precision_2": (False, 2), "hw_precision_0": (False, 0)}


def device_images(eng, size, n):
    from oracle import seres18
    from reid_amd import synth
    from reid_amd.parallel import DevArray
    base = seres18.preprocess_u8(synth.smooth_crops_u8(64, 3, *size)).numpy()
    return DevArray.from_numpy(eng, np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1, 1, 1))[:n]))


def engine():
    from reid_amd.engine import get_engine
    eng = get_engine(0)
    eng.set_precision(0)
    eng.load_seres18(*seres_weights())
    return eng


def child_trace():
    """Per size: 1024 images with hw_f16 1 twice - the first call warms up, the second is the one kernel_shares keeps."""
    from reid_amd.parallel import DevArray
    eng = engine()
    d_emb, d_log = DevArray(eng, (1024, 512), np.float32), DevArray(eng, (1024, 751), np.float32)
    for size in SIZES:
        d_x = device_images(eng, size, 1024)
        for _ in range(2):
            eng.set_hw_f16(True)
            eng.embed_f32_nchw_dev(d_x.ptr, 1024, d_emb.ptr, d_log.ptr, size=size)
            eng.set_hw_f16(False)
            eng.sync()
        d_x.free()
    eng.sync()


def short(name):
    """A trace's kernel name, mangled or not -> name or name<N>."""
    n = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", name)))
    m = re.match(r"([A-Za-z_0-9]*?_kernel)(?:ILi(\d+)|<(\d+))?", n)
    return n if not m else m.group(1) + ("<%s>" % (m.group(2) or m.group(3)) if (m.group(2) or m.group(3)) else "")


def kernel_shares(rows):
    """The trace in start order -> per size {kernel: share of the pass's kernel time}; the second hw_f16 pass of each size is the one kept."""
    passes, cur = [], None
    for name, st, en in rows:
        n = short(name)
        if "any_nchw_to_nhwc3_kernel" in n:       # every pass opens with the layout kernel (se_any_run_nchw)
            cur = collections.OrderedDict()
            passes.append(cur)
        if cur is not None:
            cur[n] = cur.get(n, 0.0) + (en - st) / 1e3
    per_size = {}
    # 1024 images: one pass at (128, 64) (pass size 4096), two at (224, 268) (pass size 545), each traced twice
    counts = {SIZES[0]: 1, SIZES[1]: 2}
    i = 0
    for size in SIZES:
        i += counts[size]                          # the warm-up
        kept = passes[i:i + counts[size]]
        i += counts[size]
        tot = collections.OrderedDict()
        for p in kept:
            for k, v in p.items():
                tot[k] = tot.get(k, 0.0) + v
        total = sum(tot.values())
        per_size["%dx%d" % size] = {"kernel_us_per_1024": round(total, 1),
                                    "share": {k: round(v / total, 4) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])}}
    if i != len(passes):
        raise RuntimeError("%d passes in the trace, expected %d" % (len(passes), i))
    return per_size


def trace_child(keep_dir):
    d = os.path.join(keep_dir, "trace_f16")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", "trace"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return dispatches(d)


def timed(eng, d_x, n, size, d_emb, d_log, launches):
    eng.sync()
    eng.timer_start()
    for _ in range(launches):
        eng.embed_f32_nchw_dev(d_x.ptr, n, d_emb.ptr, d_log.ptr, size=size)
    return eng.timer_stop() / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anysize_f16_bench.json"))
    ap.add_argument("--child", choices=["trace"], default=None)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (kernels is then reported as not taken)")
    args = ap.parse_args()
    if args.child == "trace":
        return child_trace()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (every figure comes with its spread)")

    out = {"workload": "anysize_f16: seres18_ibn seed 0, 751 classes, device-resident images, device events around "
                       "reid_embed_f32_nchw_hw_dev; %d repeats, forms alternating inside a repeat" % args.repeats, "unit": "images/s"}
    if args.no_trace:
        out["kernels"] = "not taken (--no-trace)"
    else:
        with tempfile.TemporaryDirectory() as tmp:          # the trace first: this process has not opened the device yet
            try:
                out["kernels"] = kernel_shares(trace_child(tmp))
            except (RuntimeError, subprocess.TimeoutExpired, OSError) as e:   # said in the result, never papered over
                out["kernels"] = "not taken: the trace run failed: %s" % (str(e)[-400:],)

    from reid_amd.parallel import DevArray
    from reid_amd.tracking import CameraStream
    eng = engine()
    d_emb, d_log = DevArray(eng, (1024, 512), np.float32), DevArray(eng, (1024, 751), np.float32)

    def run(form, d_x, n, size):
        f16, hp = FORMS[form]
        eng.set_hw_f16(f16)
        eng.set_hw_precision(hp)
        try:
            return timed(eng, d_x, n, size, d_emb, d_log, LAUNCHES[n])
        finally:
            eng.set_hw_f16(False)
            eng.set_hw_precision(-1)

    out["passes"], out["f16_over_x3"] = {}, {}
    for size in SIZES:
        for n in NS:
            d_x = device_images(eng, size, n)
            ms = {k: [] for k in FORMS}
            for r in range(args.repeats + 1):            # round 0 warms up (workspaces, side libraries, code objects)
                for form in FORMS:
                    t = run(form, d_x, n, size)
                    if r > 0:
                        ms[form].append(t)
            d_x.free()
            key = "%dx%d n=%d" % (size[0], size[1], n)
            out["passes"][key] = {form: dict(stats(n / (np.asarray(v) / 1e3)), ms_per_call=stats(v), calls_per_window=LAUNCHES[n])
                                  for form, v in ms.items()}
            a, b = out["passes"][key]["hw_f16"], out["passes"][key]["hw_precision_2"]
            out["f16_over_x3"][key] = {"ratio": round(a["mean"] / b["mean"], 4), "slower": bool(a["mean"] < b["mean"]),
                                       "clear": bool(abs(a["mean"] - b["mean"]) > 3 * max(a["std"], b["std"]))}

    # (256, 128) x 1024: the new forward under anysize_force against the fixed-size fp16-storage forward
    d_x = device_images(eng, (256, 128), 1024)
    ms = {"generic_hw_f16": [], "fixed_mode1": []}
    for r in range(args.repeats + 1):
        for form in ms:
            generic = form == "generic_hw_f16"
            eng.debug_switch("anysize_force", int(generic))
            eng.set_hw_f16(generic)
            eng.set_precision(0 if generic else 1)
            try:
                t = timed(eng, d_x, 1024, (256, 128), d_emb, d_log, LAUNCHES[1024])
            finally:
                eng.set_precision(0)
                eng.set_hw_f16(False)
                eng.debug_switch("anysize_force", 0)
            if r > 0:
                ms[form].append(t)
    d_x.free()
    out["generic"] = {form: dict(stats(1024 / (np.asarray(v) / 1e3)), ms_per_call=stats(v)) for form, v in ms.items()}
    out["generic"]["generic_over_fixed"] = round(out["generic"]["generic_hw_f16"]["mean"] / out["generic"]["fixed_mode1"]["mean"], 4)

    # the tracker plug-in's path: CameraStream at DeepSORT's crop size, hw_f16 against fp32-class
    s = Standin(args.frames)
    cams = {"hw_f16": CameraStream(*seres_weights(), max_dist=MAX_DIST, budget=BUDGET, arch="seres18_hw", size=SIZES[0], hw_f16=True),
            "hw_precision_f16x3": CameraStream(*seres_weights(), max_dist=MAX_DIST, budget=BUDGET, arch="seres18_hw", size=SIZES[0],
                                               hw_precision="f16x3")}
    fps = {k: [] for k in cams}
    for cam in cams.values():
        s.fill(cam.metric)
        run_stream(cam, s, 0, min(30, args.frames))
    for _ in range(args.repeats):
        for k, cam in cams.items():
            t0 = time.perf_counter()
            run_stream(cam, s, 0, args.frames)
            fps[k].append(args.frames / (time.perf_counter() - t0))
    for cam in cams.values():
        cam.close(destroy=True)
    out["stream"] = {k: dict(stats(v), unit="frames/s", path="CameraStream(arch='seres18_hw', size=(128, 64))", frames=args.frames)
                     for k, v in fps.items()}
    a, b = out["stream"]["hw_f16"], out["stream"]["hw_precision_f16x3"]
    out["stream"]["f16_over_x3"] = {"ratio": round(a["mean"] / b["mean"], 4), "slower": bool(a["mean"] < b["mean"]),
                                    "clear": bool(abs(a["mean"] - b["mean"]) > 3 * max(a["std"], b["std"]))}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
