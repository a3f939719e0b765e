"""A ResNet18-IBN-SE tracker at another crop size on the frame pipeline against the blocking calls it had before, and the fused front end
(any_front_kernel, csrc/anysize_front.hip) against the three launches it replaces.
    python tools/bench_tracking_hw.py [--frames 300] [--repeats 5] [--out profiles/tracking_hw_bench.json]
One call, one box.  The stream stand-in of bench.py's `tracking` workload (MOT16-02 is not in the container): detections per frame ~
Poisson(30) clipped to [1, 80], ragged crop sizes, 40 tracks x 100 samples, MAX_DIST 0.15; seres18_ibn seed-0 weights, hw_precision 2
(fp32-class).  Every figure is taken at (128, 64) and at (224, 268).  Prints (and writes) one JSON line, per size:
  stream      (a) frames/s of tracking.CameraStream(arch="seres18_hw"): submit / cost / fetch / update, one wait per frame
  blocking    (a) frames/s of the three blocking calls per frame such a tracker had without reid_frame_submit_hw: embed_ragged_u8(size=),
              metric.distance (gated), iou_cost on the host, metric.partial_fit - same frames, same process, a context of its own, the
              repeats of the two alternating
  pass_ms     (b) a whole pass of 30 and of 1024 crops through frame_submit_hw between two device events (reid_timer_*), switch `any_front`
              1 against 0 alternating inside each repeat; the crops are uploaded either way
  front_us    (b) the front end alone at 30 and 1024 crops: the durations of any_front_kernel (switch 1) and of any_resize_norm_kernel + the
              A_STEM_F32 GEMM + maxpool3s2_kernel (switch 0) per pass, from the device timestamps of a kernel trace of --child front
  pass_trace  (c) what the front end and the rest of a 30-crop pass cost at switch 1 and 0, from the same trace
Each figure is the mean over --repeats repeats with their standard deviation, minimum and maximum.  The traces are `rocprofv3
--kernel-trace --stats` runs of this file (--child front: a fresh process started before this one touches the device, no counters); (a)
and pass_ms are taken afterwards with the profiler off.  `verdict`: per (size, crops), whether any_front_kernel is faster than the three
launches by more than three times the larger standard deviation."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tracking_swin import BUDGET, MAX_DIST, TRACKS, dispatches, stats  # noqa: E402

SIZES = ((128, 64), (224, 268))
PASSES = (30, 1024)
PASS_LAUNCHES, PASS_WARMUP = 4, 1
# the kernels of the two front ends (A_STEM_F32 = 2, reid_internal.h: the stem is the only launch of that build in a pass at hw_precision 2)
FRONT = {1: ("any_front_kernel",), 0: ("any_resize_norm_kernel", "gemm_f32_kernel<2,", "gemm_f32_kernelILi2E", "maxpool3s2_kernel")}
FRONT_LAUNCHES = {1: 1, 0: 3}


class Standin:
    """bench.py run_tracking's frames: counts, crop pool, boxes, and the bank's initial samples."""

    def __init__(self, frames):
        from reid_amd import synth
        rng = np.random.default_rng(3)
        self.frames = frames
        self.counts = np.clip(rng.poisson(30, frames), 1, 80)
        self.pool = synth.ragged_crops_u8(256, seed=3)
        self.tracks = list(range(TRACKS))
        self.seed_feats = rng.normal(size=(TRACKS * BUDGET, 512)).astype(np.float32)
        self.boxes = rng.uniform(0, 500, (80, 4))
        self.boxes[:, 2:] = rng.uniform(20, 120, (80, 2))

    def crops_of(self, f):
        return [self.pool[(f * 7 + i) % 256] for i in range(int(self.counts[f]))]

    def batch(self, n):
        return [self.pool[i % 256] for i in range(n)]

    def fill(self, metric):
        metric.partial_fit(self.seed_feats, np.repeat(self.tracks, BUDGET), self.tracks)


def seres_weights():
    from reid_amd import synth, weights
    return weights.pack_seres18(synth.seres18_state_dict(0))[:2]


def run_stream(cam, s, first, last):
    cam.submit(s.crops_of(first))
    for f in range(first, last):
        n = int(s.counts[f])
        nxt = s.crops_of(f + 1) if f + 1 < last else None
        cam.step(s.tracks, s.boxes[:TRACKS], s.boxes[:n], nxt)
        k = min(n, TRACKS)
        cam.commit(np.arange(k), s.tracks[:k], s.tracks)
    cam.eng.sync()


def run_blocking(eng, metric, s, size, first, last):
    from reid_amd.iou_matching import iou_cost
    for f in range(first, last):
        n = int(s.counts[f])
        feats = eng.embed_ragged_u8(s.crops_of(f), size=size)
        metric.distance(feats, s.tracks, max_distance=MAX_DIST)
        iou_cost(s.boxes[:TRACKS], s.boxes[:n])
        k = min(n, TRACKS)
        metric.partial_fit(feats[:k], s.tracks[:k], s.tracks)
    eng.sync()


def one_pass(eng, crops, size):
    eng.frame_submit_hw(0, crops, size)
    eng.frame_cost(0, want_emb=False)
    eng.frame_fetch(0)


def front_engine():
    from reid_amd.engine import get_engine
    eng = get_engine(0)
    eng.load_seres18(*seres_weights())
    eng.set_hw_precision(2)
    return eng


# ------------------------------------------------------------------------------------------------ child (under rocprofv3)
def child_front(repeats):
    """Per size and pass size: a warm-up, then repeats x (PASS_LAUNCHES passes at any_front 1, as many at 0)."""
    eng = front_engine()
    s = Standin(1)
    for size in SIZES:
        for n in PASSES:
            crops = s.batch(n)
            for r in range(-1, repeats):
                for sw in (1, 0):
                    eng.debug_switch("any_front", sw)
                    for _ in range(PASS_WARMUP if r < 0 else PASS_LAUNCHES):
                        one_pass(eng, crops, size)
    eng.debug_switch("any_front", 2)
    eng.sync()


def front_from_trace(rows, repeats):
    """The trace in start order -> {size: {crops: {switch: stats of the front end's us per pass}}} and the 30-crop pass split.  A segment is
    the kernels between two runs of front-end kernels of the other switch: the child's loop order is known, the segments are counted."""
    from reid_amd.engine import any_pass_size
    is_front = {sw: (lambda n, names=names: any(k in n for k in names)) for sw, names in FRONT.items()}
    segs, cur = [], None            # [switch, front us, rest us, front launches]
    for name, st, en in rows:
        sw = 1 if is_front[1](name) else (0 if is_front[0](name) else None)
        if sw is not None and (cur is None or cur[0] != sw):
            cur = [sw, 0.0, 0.0, 0]
            segs.append(cur)
        if cur is None:
            continue                # weight loading
        if sw is None:
            cur[2] += (en - st) / 1e3
        else:
            cur[1] += (en - st) / 1e3
            cur[3] += 1
    want = len(SIZES) * len(PASSES) * (repeats + 1) * 2
    if len(segs) != want:
        raise RuntimeError("%d front-end segments in the trace, expected %d" % (len(segs), want))
    out, split, i = {}, {}, 0
    for size in SIZES:
        key = "%dx%d" % size
        out[key], split[key] = {}, {}
        for n in PASSES:
            sub = (n + any_pass_size(1024, *size) - 1) // any_pass_size(1024, *size)
            per = {1: [], 0: []}
            rest = {1: [], 0: []}
            for r in range(-1, repeats):
                for sw in (1, 0):
                    seg = segs[i]
                    i += 1
                    launches = (PASS_WARMUP if r < 0 else PASS_LAUNCHES)
                    if seg[0] != sw or seg[3] != launches * sub * FRONT_LAUNCHES[sw]:
                        raise RuntimeError("segment %d: switch %d with %d front-end launches, expected switch %d with %d" %
                                           (i - 1, seg[0], seg[3], sw, launches * sub * FRONT_LAUNCHES[sw]))
                    if r >= 0:
                        per[sw].append(seg[1] / launches)
                        rest[sw].append(seg[2] / launches)
            out[key][str(n)] = {"any_front_1": dict(stats(per[1]), unit="us per pass, any_front_kernel"),
                                "any_front_0": dict(stats(per[0]), unit="us per pass, resize + stem GEMM + max-pool")}
            if n == PASSES[0]:
                split[key] = {"front_us": {"any_front_1": stats(per[1]), "any_front_0": stats(per[0])},
                              "rest_of_pass_us": {"any_front_1": stats(rest[1]), "any_front_0": stats(rest[0])},
                              "note": "kernel time of a %d-crop pass from the trace: the front end, and every other kernel of the pass" % n}
    return out, split


def trace_child(repeats, keep_dir):
    d = os.path.join(keep_dir, "trace_front")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", "front",
           "--repeats", str(repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return dispatches(d)


def pass_ms(eng, s, size, n, repeats):
    crops = s.batch(n)
    out = {1: [], 0: []}
    for r in range(-1, repeats):
        for sw in (1, 0):
            eng.debug_switch("any_front", sw)
            eng.sync()
            eng.timer_start()
            for _ in range(PASS_WARMUP if r < 0 else PASS_LAUNCHES):
                eng.frame_submit_hw(0, crops, size)
            ms = eng.timer_stop() / (PASS_WARMUP if r < 0 else PASS_LAUNCHES)
            if r >= 0:
                out[sw].append(ms)
    eng.debug_switch("any_front", 2)
    return {"any_front_1": dict(stats(out[1]), unit="ms per pass"), "any_front_0": dict(stats(out[0]), unit="ms per pass")}


def faster(a, b):
    """a (fused) faster than b by more than three of the larger standard deviation"""
    return bool(b["mean"] - a["mean"] > 3.0 * max(a["std"], b["std"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["front"], default=None)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (front_us and pass_trace are then reported as not taken)")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (every figure comes with its spread)")
    if args.child == "front":
        return child_front(args.repeats)

    out = {"workload": "stream stand-in of bench.py --workload tracking: %d frames per repeat, Poisson(30) ragged crops, %d tracks x %d samples, "
                       "seres18_ibn seed 0, hw_precision 2 (fp32-class), MAX_DIST %.2f; %d repeats" % (args.frames, TRACKS, BUDGET, MAX_DIST, args.repeats)}
    if args.no_trace:
        out["front_us"] = out["pass_trace"] = "not taken (--no-trace)"
    else:
        with tempfile.TemporaryDirectory() as tmp:          # the trace first: this process has not opened the device yet
            out["front_us"], out["pass_trace"] = front_from_trace(trace_child(args.repeats, tmp), args.repeats)

    from reid_amd.engine import Engine
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    from reid_amd.tracking import CameraStream
    s = Standin(args.frames)
    eng = front_engine()
    out["pass_ms"] = {"%dx%d" % size: {str(n): pass_ms(eng, s, size, n, args.repeats) for n in PASSES} for size in SIZES}
    eng.set_hw_precision(-1)
    out["stream"], out["blocking"] = {}, {}
    for size in SIZES:
        cam = CameraStream(*seres_weights(), max_dist=MAX_DIST, budget=BUDGET, arch="seres18_hw", size=size, hw_precision=2)
        s.fill(cam.metric)
        beng = Engine(0)
        beng.load_seres18(*seres_weights())
        beng.set_hw_precision(2)
        bmetric = NearestNeighborDistanceMetric("cosine", MAX_DIST, BUDGET, engine=beng)
        s.fill(bmetric)
        warm = min(30, args.frames)
        run_stream(cam, s, 0, warm)
        run_blocking(beng, bmetric, s, size, 0, warm)
        fps = {"stream": [], "blocking": []}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            run_stream(cam, s, 0, args.frames)
            fps["stream"].append(args.frames / (time.perf_counter() - t0))
            t0 = time.perf_counter()
            run_blocking(beng, bmetric, s, size, 0, args.frames)
            fps["blocking"].append(args.frames / (time.perf_counter() - t0))
        cam.close(destroy=True)
        bmetric.close()
        beng.close()
        key = "%dx%d" % size
        out["stream"][key] = dict(stats(fps["stream"]), unit="frames/s", path="CameraStream(arch='seres18_hw')")
        out["blocking"][key] = dict(stats(fps["blocking"]), unit="frames/s", path="embed_ragged_u8(size=) + metric.distance + iou_cost + metric.partial_fit")
    verdict = {}
    for size in SIZES:
        key = "%dx%d" % size
        for n in PASSES:
            p = out["pass_ms"][key][str(n)]
            v = {"pass_ms_fused_faster_by_3_sigma": faster(p["any_front_1"], p["any_front_0"])}
            if not args.no_trace:
                fr = out["front_us"][key][str(n)]
                v["front_us_fused_faster_by_3_sigma"] = faster(fr["any_front_1"], fr["any_front_0"])
            verdict["%s n=%d" % (key, n)] = v
    out["verdict"] = verdict
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
