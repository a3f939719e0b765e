"""The evaluation chain's first link on the device: descriptors from uint8 images as the dataset stores them (reid_descriptor_images_u8,
reid_swin_descriptor_images_u8) beside the float entries on images that were already preprocessed on the host.
    python tools/bench_pil_resize.py [--n 1024] [--repeats 5] [--out profiles/pil_resize_bench.json]
One call, one box.  Two workloads of n images:
  market   n Market-1501-size images, 128 x 64 (64 distinct synth images tiled: the content does not change the work)
  ragged   n images with h = 100 + 37 i mod 301 (100 .. 400) and w = 40 + 53 i mod 161 (40 .. 200)
and two backbones in the fp32-class mode (2) with seed-0 weights and 751 classes, mirrored view on: ResNet18-IBN-SE at 256 x 128 and
Swin-T v1 at 448 x 224.  Prints (and writes) one JSON line:
  <backbone>.<workload>.images_u8   descriptors/s of the new entry, host uint8 in, host descriptors out
  <backbone>.<workload>.f32_nchw    descriptors/s of reid_descriptor_f32_nchw / reid_swin_descriptor_f32_nchw on the SAME images as
                                    preprocessed host floats (the host preprocessing itself - about 1 ms per image with PIL - is NOT in
                                    this figure: it is what the caller of the float entry pays on top)
  <backbone>.<workload>.bit_equal   the two results are the same bits
  <backbone>.<workload>.host_pack_ms  what Engine._pack_images takes on its own: images that lie one after the other in one buffer (market)
                                    are handed over in place, a list of separate arrays (ragged) is copied into one buffer first; this
                                    time is part of images_u8's
  resize_kernels.<size>.<workload>  the two resize kernels' time per launch of n images, from ONE `rocprofv3 --kernel-trace --stats` run of
                                    this file (--child trace, a fresh process started before this one touches the device)
  slower_than_float_entry           the (backbone, workload) pairs where the new entry's mean rate is below the float entry's
Each rate is the mean over --repeats repeats with standard deviation, minimum and maximum; one warm-up round first; the repeats of the two
entries alternate.  Reported as measured: there is no threshold."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_tracking_swin import dispatches, stats  # noqa: E402

SIZES = {"seres18": (256, 128), "swin": (448, 224)}
KERNELS = ("pil_resize_h_kernel", "pil_resize_v_kernel")


def workloads(n):
    from reid_amd import synth
    base = synth.smooth_crops_u8(64, seed=3, h=128, w=64)
    market = np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1, 1, 1))[:n])
    noise = np.random.default_rng(7).integers(0, 256, (400, 200, 3), dtype=np.uint8)
    ragged = [np.ascontiguousarray(noise[:100 + (37 * i) % 301, :40 + (53 * i) % 161]) for i in range(n)]
    return {"market": list(market), "ragged": ragged}


def child_trace(n, repeats):
    """Under rocprofv3: per output size and workload one warm-up launch and `repeats` launches of all n images through the launcher the
    entries call (reid_debug_pil_resize without the uint8 output, as the entries launch it)."""
    from reid_amd.engine import get_engine
    eng = get_engine(0)
    wl = workloads(n)
    for size in SIZES.values():
        for images in wl.values():
            for _ in range(repeats + 1):
                eng.debug_pil_resize(images, size, want_u8=False)


def resize_kernels(n, repeats, tmp):
    d = os.path.join(tmp, "trace")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", "trace",
           "--n", str(n), "--repeats", str(repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    rows = [(name, (e - s) / 1e3) for name, s, e in dispatches(d) if any(k in name for k in KERNELS)]
    configs = [(b, w) for b in SIZES for w in ("market", "ragged")]
    if len(rows) != len(configs) * (repeats + 1) * 2:
        raise RuntimeError("%d resize launches in the trace, expected %d" % (len(rows), len(configs) * (repeats + 1) * 2))
    out = {}
    for c, (b, w) in enumerate(configs):
        part = rows[c * (repeats + 1) * 2 + 2:(c + 1) * (repeats + 1) * 2]               # without the warm-up pair
        hs = [us for name, us in part if KERNELS[0] in name]
        vs = [us for name, us in part if KERNELS[1] in name]
        assert len(hs) == len(vs) == repeats
        out.setdefault("%dx%d" % SIZES[b], {})[w] = {"horizontal_us": stats(hs), "vertical_us": stats(vs),
                                                     "both_us_per_image": round((np.mean(hs) + np.mean(vs)) / n, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pil_resize_bench.json"))
    ap.add_argument("--child", choices=["trace"], default=None)
    args = ap.parse_args()
    if args.child == "trace":
        return child_trace(args.n, args.repeats)
    n = args.n
    out = {"workload": "pil_resize", "n": n, "precision": 2, "num_class": 751, "flip_tta": True, "unit": "descriptors/s", "repeats": args.repeats}
    with tempfile.TemporaryDirectory() as tmp:              # the trace first: this process has not opened the device yet
        out["resize_kernels"] = resize_kernels(n, args.repeats, tmp)

    from reid_amd import synth, weights
    from reid_amd.engine import get_engine
    eng = get_engine(0)
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    eng.set_precision(2)
    wl = workloads(n)
    slower = []
    for backbone, size in SIZES.items():
        new = eng.descriptor_images_u8 if backbone == "seres18" else (lambda im: eng.swin_descriptor_images_u8(im, size=size))
        old = eng.descriptor_f32_nchw if backbone == "seres18" else eng.swin_descriptor_f32_nchw
        out[backbone] = {"size": list(size)}
        for name, images in wl.items():
            pre = eng.debug_pil_resize(images, size, want_u8=False)[1]          # the preprocessed host floats the float entry is given
            runs = {"images_u8": lambda: new(images), "f32_nchw": lambda: old(pre)}
            rates, results = {k: [] for k in runs}, {}
            for r in range(args.repeats + 1):                                    # round 0 warms up (workspaces, the side library)
                for k, fn in runs.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    results[k] = fn()
                    if r:
                        rates[k].append(n / (time.perf_counter() - t0))
            row = {k: stats(v) for k, v in rates.items()}
            pack = []
            for _ in range(args.repeats):                                        # the host-side packing of the list alone (inside images_u8's time)
                t0 = time.perf_counter()
                eng._pack_images(images)
                pack.append((time.perf_counter() - t0) * 1e3)
            row["host_pack_ms"] = stats(pack)
            row["bit_equal"] = bool(np.array_equal(results["images_u8"].view(np.uint32), results["f32_nchw"].view(np.uint32)))
            row["source_mb"] = round(sum(im.nbytes for im in images) / 1e6, 1)
            row["float_mb"] = round(pre.nbytes / 1e6, 1)
            out[backbone][name] = row
            if row["images_u8"]["mean"] < row["f32_nchw"]["mean"]:
                slower.append("%s/%s" % (backbone, name))
            pre = None
    out["slower_than_float_entry"] = slower
    line = json.dumps(out)
    print(line)
    print("new entry slower than the float entry on already-preprocessed floats: %s" % (", ".join(slower) if slower else "nowhere"), file=sys.stderr)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
