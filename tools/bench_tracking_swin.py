"""A Swin-T tracker on the frame pipeline against the blocking calls it had before, and the 96-wide cost kernel against the generic one.
    python tools/bench_tracking_swin.py [--frames 300] [--repeats 5] [--out profiles/tracking_swin_bench.json]
One call, one box.  The stream stand-in of bench.py's `tracking` workload (MOT16-02 is not in the container): detections per frame ~
Poisson(30) clipped to [1, 80], ragged crop sizes, 40 tracks x 100 samples, MAX_DIST 0.15; Swin-T v1, seed-0 weights, fp32-class
arithmetic (mode 2), crops resized to 224x224.  Prints (and writes) one JSON line:
  stream         (a) frames/s of tracking.CameraStream(arch="swin"): submit / cost / fetch / update, one wait per frame
  blocking       (b) frames/s of the three blocking calls per frame a Swin tracker had without reid_frame_submit_swin:
                 swin_embed_ragged_u8, metric.distance (gated), iou_cost on the host, metric.partial_fit - same frames, same process,
                 a context of its own, the repeats of (a) and (b) alternating
  cost_stage     (c) kernel time of the cost stage at 40 tracks x 100 samples x 30 detections with the `bank_fast` switch at 1
                 (bank_cost96_kernel) and 0 (bank_cost_kernel), through reid_debug_bank_cost96, from a kernel trace
  frame_kernels  kernel time per frame of the stream (all kernels of 40 frames over 40), from a second kernel trace
Each figure is the mean over --repeats repeats with their standard deviation, minimum and maximum.  (c) and frame_kernels come from
`rocprofv3 --kernel-trace --stats` runs of this file (--child cost / --child frames: fresh processes started before this one touches the
device, no counters); (a) and (b) are taken afterwards with the profiler off.  `accept` states the two comparisons: (a) not slower than
(b) beyond (b)'s spread; bank_cost96_kernel faster than bank_cost_kernel by more than the two spreads combined."""
import argparse
import csv
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRACKS, BUDGET, MAX_DIST, DETS = 40, 100, 0.15, 30
COST_LAUNCHES, COST_WARMUP, TRACE_FRAMES = 20, 3, 40


def stats(v):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), 4), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 4), "min": round(float(v.min()), 4),
            "max": round(float(v.max()), 4), "n": int(len(v))}


class Standin:
    """bench.py run_tracking's frames: counts, crop pool, boxes, and the bank's initial samples (96 wide here)."""

    def __init__(self, frames):
        from reid_amd import synth
        rng = np.random.default_rng(3)
        self.frames = frames
        self.counts = np.clip(rng.poisson(30, frames), 1, 80)
        self.pool = synth.ragged_crops_u8(256, seed=3)
        self.tracks = list(range(TRACKS))
        self.seed_feats = rng.normal(size=(TRACKS * BUDGET, 96)).astype(np.float32)
        self.boxes = rng.uniform(0, 500, (80, 4))
        self.boxes[:, 2:] = rng.uniform(20, 120, (80, 2))

    def crops_of(self, f):
        return [self.pool[(f * 7 + i) % 256] for i in range(int(self.counts[f]))]

    def fill(self, metric):
        metric.partial_fit(self.seed_feats, np.repeat(self.tracks, BUDGET), self.tracks)


def swin_weights():
    from reid_amd import synth, weights
    return weights.pack_swin(synth.swin_state_dict(0))[:2]


def run_stream(cam, s, first, last):
    cam.submit(s.crops_of(first))
    for f in range(first, last):
        n = int(s.counts[f])
        nxt = s.crops_of(f + 1) if f + 1 < last else None
        cam.step(s.tracks, s.boxes[:TRACKS], s.boxes[:n], nxt)
        k = min(n, TRACKS)
        cam.commit(np.arange(k), s.tracks[:k], s.tracks)
    cam.eng.sync()


def run_blocking(eng, metric, s, first, last):
    from reid_amd.iou_matching import iou_cost
    for f in range(first, last):
        n = int(s.counts[f])
        feats = eng.swin_embed_ragged_u8(s.crops_of(f))
        metric.distance(feats, s.tracks, max_distance=MAX_DIST)
        iou_cost(s.boxes[:TRACKS], s.boxes[:n])
        k = min(n, TRACKS)
        metric.partial_fit(feats[:k], s.tracks[:k], s.tracks)
    eng.sync()


def make_stream(s):
    from reid_amd.tracking import CameraStream
    cam = CameraStream(*swin_weights(), precision=2, max_dist=MAX_DIST, budget=BUDGET, arch="swin")
    s.fill(cam.metric)
    return cam


# ------------------------------------------------------------------------------------------------ children (under rocprofv3)
def child_cost(repeats):
    """repeats x (COST_LAUNCHES launches with bank_fast 1, then as many with 0) of the cost stage at TRACKS x BUDGET x DETS."""
    from reid_amd import _ffi
    from reid_amd.engine import get_engine
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    eng = get_engine(0)
    s = Standin(1)
    metric = NearestNeighborDistanceMetric("cosine", MAX_DIST, BUDGET, engine=eng)
    s.fill(metric)
    slots = metric._slots_for(s.tracks, False)
    dets = np.random.default_rng(4).normal(size=(DETS, 96)).astype(np.float32)
    out = {}
    for r in range(-1, repeats):                     # -1: warm-up, COST_WARMUP launches each
        for fast in (1, 0):
            eng.debug_switch("bank_fast", fast)
            for _ in range(COST_WARMUP if r < 0 else COST_LAUNCHES):
                out[fast] = eng.debug_bank_cost96(metric._bank, slots, dets, _ffi.METRIC_COS, MAX_DIST)
    eng.debug_switch("bank_fast", 1)
    assert np.abs(out[1].astype(np.float64) - out[0]).max() < 1e-5


def child_frames():
    s = Standin(TRACE_FRAMES + 8)
    cam = make_stream(s)
    run_stream(cam, s, 0, 8)                           # warm-up: not separated in the trace, 8 frames of 48
    run_stream(cam, s, 8, TRACE_FRAMES + 8)
    cam.close(destroy=True)


def dispatches(trace_dir):
    """[(kernel name, start ns, end ns)] of a rocprofv3 --kernel-trace output directory, in start order: the rocpd database, or the CSV."""
    rows = []
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        c = sqlite3.connect(db)
        tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")]
        if kd and ks:
            rows += c.execute("select s.kernel_name, d.start, d.end from %s d join %s s on d.kernel_id=s.id" % (kd[0], ks[0])).fetchall()
    if not rows:
        for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    if not rows:
        raise RuntimeError("no kernel dispatches found under %s: %s" % (trace_dir, os.listdir(trace_dir)))
    return sorted(rows, key=lambda r: r[1])


def trace_child(which, repeats, keep_dir):
    d = os.path.join(keep_dir, "trace_" + which)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", which,
           "--repeats", str(repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return dispatches(d)


def cost_stage(rows, repeats):
    out = {}
    for key, name in (("bank_fast_1", "bank_cost96_kernel"), ("bank_fast_0", "bank_cost_kernel")):
        us = np.array([(e - s) / 1e3 for n, s, e in rows if name in n])
        if len(us) != COST_WARMUP + repeats * COST_LAUNCHES:
            raise RuntimeError("%s: %d launches in the trace, expected %d" % (name, len(us), COST_WARMUP + repeats * COST_LAUNCHES))
        per = us[COST_WARMUP:].reshape(repeats, COST_LAUNCHES).mean(1)
        out[key] = dict(stats(per), kernel=name, unit="us per launch, mean of %d launches per repeat" % COST_LAUNCHES)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["cost", "frames"], default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (every figure comes with its spread)")
    if args.child == "cost":
        return child_cost(args.repeats)
    if args.child == "frames":
        return child_frames()

    out = {"workload": "stream stand-in of bench.py --workload tracking: %d frames per repeat, Poisson(30) ragged crops, %d tracks x %d samples, "
                       "Swin-T v1 seed 0, fp32-class (mode 2), 224x224, MAX_DIST %.2f; %d repeats" % (args.frames, TRACKS, BUDGET, MAX_DIST, args.repeats)}
    with tempfile.TemporaryDirectory() as tmp:          # the traces first: this process has not opened the device yet
        out["cost_stage"] = cost_stage(trace_child("cost", args.repeats, tmp), args.repeats)
        rows = trace_child("frames", args.repeats, tmp)
    total_us = sum(e - s for _, s, e in rows) / 1e3
    by = {}
    for n, s, e in rows:
        by[n] = by.get(n, 0.0) + (e - s) / 1e3
    top = sorted(by.items(), key=lambda kv: -kv[1])[:8]
    out["frame_kernels"] = {"us_per_frame": round(total_us / (TRACE_FRAMES + 8), 1), "launches_per_frame": round(len(rows) / (TRACE_FRAMES + 8), 1),
                            "frames": TRACE_FRAMES + 8, "note": "all kernels of the traced stream (bank seeding included) over its frames; one run, no spread",
                            "top_us_per_frame": {n[:80]: round(v / (TRACE_FRAMES + 8), 1) for n, v in top}}

    from reid_amd.engine import Engine
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    s = Standin(args.frames)
    cam = make_stream(s)
    beng = Engine(0)
    beng.load_swin(*swin_weights())
    beng.set_precision(2)
    bmetric = NearestNeighborDistanceMetric("cosine", MAX_DIST, BUDGET, engine=beng)
    s.fill(bmetric)
    warm = min(30, args.frames)
    run_stream(cam, s, 0, warm)
    run_blocking(beng, bmetric, s, 0, warm)
    fps = {"stream": [], "blocking": []}
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        run_stream(cam, s, 0, args.frames)
        fps["stream"].append(args.frames / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        run_blocking(beng, bmetric, s, 0, args.frames)
        fps["blocking"].append(args.frames / (time.perf_counter() - t0))
    cam.close(destroy=True)
    bmetric.close()
    beng.close()
    out["stream"] = dict(stats(fps["stream"]), unit="frames/s", path="CameraStream(arch='swin')")
    out["blocking"] = dict(stats(fps["blocking"]), unit="frames/s", path="swin_embed_ragged_u8 + metric.distance + iou_cost + metric.partial_fit")
    f1, f0 = out["cost_stage"]["bank_fast_1"], out["cost_stage"]["bank_fast_0"]
    out["accept"] = {"stream_not_slower_than_blocking_beyond_its_spread": bool(out["stream"]["mean"] >= out["blocking"]["mean"] - out["blocking"]["std"]),
                     "cost96_beats_generic_by_more_than_both_spreads": bool(f1["mean"] + f1["std"] + f0["std"] < f0["mean"])}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
