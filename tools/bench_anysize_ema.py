"""EMARes18-IBN at another input size: what the EMA tail of libreid_hip_anysize_ema.so costs, against the slab-in-LDS kernel of the
256 x 128 forward (ema_tail_kernel, csrc/attention_f32.hip) in the same trunk and against seres18_ibn and cares18_ibn through the same entry.
    python tools/bench_anysize_ema.py [--repeats 5] [--no-trace] [--out profiles/anysize_ema_bench.json]
One call, one box (boxes of a pool differ by several per cent: figures of different calls are not compared).  Seed-0 weights with 751
classes, images resident on the device (64 distinct images tiled to n: the content does not change the work), embeddings and logits
left there: device events around reid_embed_f32_nchw_hw_dev, so neither PCIe nor numpy is in the figure.  Prints (and writes) one JSON line;
every rate is the mean over --repeats repeats with their standard deviation, minimum and maximum, one warm-up round first, the repeats of
the forms alternating.  Per size (224 x 268, the script's VeRi geometry; 128 x 64, a DeepSORT crop - at both the old kernel's slab still
fits LDS), pass (1024 and 30 images) and reid_ctx_set_hw_precision (0 exact fp32, 2 fp32-class):
  ema_new   images/s of emares18_ibn, reid_ctx_set_hw_ema 1, debug switch any_ema 1 (the new library)
  ema_old   the same with any_ema 0 (ema_tail_kernel in the any-size trunk)
  se, ca    seres18_ibn, and cares18_ibn with reid_ctx_set_hw_siblings 1, through the same entry: the reference points
  new_over_old   the ratio of the means, and `clear` = the means differ by more than three of the larger standard deviation
  tail_share     from ONE `rocprofv3 --kernel-trace --stats` run of a child process of its own (one warm-up and one measured call per form,
                 exact fp32): the share of the call's kernel time that the tail's kernels take, new (any_ema_*) and old (ema_tail_kernel),
                 and the tail's time per call in ms - whether the old tail's cost is the tail itself
Reported as measured: there is no threshold."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((224, 268), (128, 64))
PASSES = (1024, 30)


def stats(v, digits=1):
    v = np.asarray(v, np.float64)
    return {"mean": round(float(v.mean()), digits), "std": round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, digits),
            "min": round(float(v.min()), digits), "max": round(float(v.max()), digits), "n": int(len(v))}


def setup():
    from oracle import seres18
    from reid_amd import synth, weights
    from reid_amd.engine import get_engine
    from reid_amd.parallel import DevArray
    eng = get_engine(0)
    eng.set_precision(0)
    blobs = {"se": weights.pack_seres18(synth.seres18_state_dict(0))[:2], "ca": weights.pack_seres18(synth.cares18_state_dict(0))[:2],
             "ema": weights.pack_seres18(synth.emares18_state_dict(0))[:2]}
    nmax = max(PASSES)
    d_emb, d_log = DevArray(eng, (nmax, 512), np.float32), DevArray(eng, (nmax, 751), np.float32)
    d_x = {}
    for h, w in SIZES:
        base = seres18.preprocess_u8(synth.smooth_crops_u8(64, 3, h, w)).numpy()
        d_x[(h, w)] = DevArray.from_numpy(eng, np.ascontiguousarray(np.tile(base, ((nmax + 63) // 64, 1, 1, 1))[:nmax]))

    def run(size, n, hw_precision, any_ema):
        eng.debug_switch("any_ema", any_ema)
        eng.set_hw_precision(hw_precision)
        try:
            eng.timer_start()
            eng.embed_f32_nchw_dev(d_x[size].ptr, n, d_emb.ptr, d_log.ptr, size=size)
            return eng.timer_stop()
        finally:
            eng.set_hw_precision(-1)
            eng.debug_switch("any_ema", 1)
    return eng, blobs, run


def child_trace():
    """Under rocprofv3: emares18_ibn in exact fp32, per (size, pass) the new tail twice, then the old tail twice (the first of each warms
    up).  The parent splits the trace by these counts."""
    eng, blobs, run = setup()
    eng.load_seres18(*blobs["ema"])
    eng.set_hw_ema(True)
    for size in SIZES:
        for n in PASSES:
            for any_ema in (1, 0):
                for _ in range(2):
                    run(size, n, 0, any_ema)
    eng.sync()


def tail_share(tmp):
    from bench_tracking_swin import dispatches
    d = os.path.join(tmp, "trace")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child", "trace"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s -> %d\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    rows = [(name, (e - s) / 1e6) for name, s, e in dispatches(d)]
    # a call's tail launches: 8 blocks per pass, four kernels a block (new) or one (old); calls are told apart by the child's order
    from reid_amd.engine import any_pass_size
    tails = [(name, ms) for name, ms in rows if "any_ema_" in name or "ema_tail_kernel" in name]
    out, total_by_kind, pos = {}, {}, 0
    for size in SIZES:
        for n in PASSES:
            passes = -(-n // min(n, any_pass_size(1024, *size)))
            for kind, per_block in (("new", 4), ("old", 1)):
                count = 8 * per_block * passes
                part = tails[pos + count:pos + 2 * count]                       # the second call: the first warmed up
                pos += 2 * count
                want = "any_ema_" if kind == "new" else "ema_tail_kernel"
                if len(part) != count or not all(want in name for name, _ in part):
                    raise RuntimeError("the trace does not hold the child's calls in order at %s x %d (%s)" % (size, n, kind))
                total_by_kind[(size, n, kind)] = sum(ms for _, ms in part)
    # the trace gives the tail's own time; the whole call's time is the device-event figure of the main run
    for size in SIZES:
        for n in PASSES:
            out["%dx%d_n%d" % (size[0], size[1], n)] = {"new_tail_ms": round(total_by_kind[(size, n, "new")], 4),
                                                        "old_tail_ms": round(total_by_kind[(size, n, "old")], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (tail_share is then reported as not taken)")
    ap.add_argument("--child", choices=["trace"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anysize_ema_bench.json"))
    args = ap.parse_args()
    if args.child == "trace":
        return child_trace()
    trace, trace_note = None, "not taken"
    if not args.no_trace:                                    # the trace first: this process has not opened the device yet
        try:
            with tempfile.TemporaryDirectory() as tmp:
                trace = tail_share(tmp)
            trace_note = "rocprofv3 --kernel-trace --stats, one run of a child process"
        except (RuntimeError, OSError, subprocess.SubprocessError) as e:      # the rates below do not depend on it
            trace_note = "not taken: %s" % (str(e)[:300],)
    from reid_amd.engine import any_pass_size
    eng, blobs, run = setup()
    forms = [(size, n, p) for size in SIZES for n in PASSES for p in (0, 2)]
    kinds = ("ema_new", "ema_old", "se", "ca")
    ms = {(f, which): [] for f in forms for which in kinds}
    try:
        for r in range(args.repeats + 1):            # round 0 warms up (workspaces, the side libraries, code objects)
            for arch in ("ema", "se", "ca"):         # one load per architecture and round
                eng.load_seres18(*blobs[arch])
                eng.set_hw_ema(arch == "ema")
                eng.set_hw_siblings(arch == "ca")
                for f in forms:
                    for which, any_ema in ((("ema_new", 1), ("ema_old", 0)) if arch == "ema" else ((arch, 1),)):
                        t = run(f[0], f[1], f[2], any_ema)
                        if r > 0:
                            ms[(f, which)].append(t)
        eng.sync()
    finally:
        eng.set_hw_ema(False)
        eng.set_hw_siblings(False)
    out = {"workload": "anysize_ema", "num_class": 751, "unit": "images/s", "repeats": args.repeats, "results": []}
    slower = []
    for size, n, p in forms:
        row = {"size": list(size), "n": n, "hw_precision": p, "pass_images": min(n, any_pass_size(1024, *size))}
        for which in kinds:
            t = np.asarray(ms[((size, n, p), which)])
            row[which] = stats(n / (t / 1e3))
            row[which]["ms_per_call"] = stats(t, 3)
        a, b = row["ema_new"], row["ema_old"]
        row["new_over_old"] = {"ratio": round(a["mean"] / b["mean"], 4), "clear": bool(abs(a["mean"] - b["mean"]) > 3 * max(a["std"], b["std"]))}
        row["ema_new_over_se"] = round(a["mean"] / row["se"]["mean"], 4)
        row["ema_new_over_ca"] = round(a["mean"] / row["ca"]["mean"], 4)
        if p == 0 and trace is not None:
            tr = trace["%dx%d_n%d" % (size[0], size[1], n)]
            row["tail_share"] = {"new_tail_ms": tr["new_tail_ms"], "old_tail_ms": tr["old_tail_ms"],
                                 "new_share_of_call": round(tr["new_tail_ms"] / a["ms_per_call"]["mean"], 4),
                                 "old_share_of_call": round(tr["old_tail_ms"] / b["ms_per_call"]["mean"], 4)}
        if row["new_over_old"]["clear"] and row["new_over_old"]["ratio"] < 1.0:
            slower.append({"size": list(size), "n": n, "hw_precision": p, "ratio": row["new_over_old"]["ratio"]})
        out["results"].append(row)
    out["new_slower_than_old"] = slower
    out["tail_trace"] = trace_note
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
