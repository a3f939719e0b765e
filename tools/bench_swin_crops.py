"""Swin-T fed the tracker's way: uint8 crops of any size through reid_swin_embed_ragged_u8, beside the device-resident float path.
    python tools/bench_swin_crops.py [--out profiles/swin_crops_bench.json]
One process, one call, one box, fp32-class arithmetic (mode 2), Swin-T v1, seed-0 weights.  Prints (and writes) one JSON line:
  resident     images/s of reid_swin_embed_f32_nchw_dev on 1024 device-resident 224x224 images: the unchanged float path, the yardstick
  ragged_*     images/s of reid_swin_embed_ragged_u8 on 4096 ragged host crops (heights log-uniform in [40, 400], w = h U(0.3, 0.5), as
               tools/bench_tracking.py draws them), host in -> host out, from a pinned slab and from pageable memory, with the host
               pipeline (the default) and without it (upload, passes, download one after the other: what the overlap hides), each with
               its ratio to `resident`
  kernels      the fused front kernel's own time on 1024 of these crops beside sfe_conv1_kernel's on 1024 images (each alone through its
               harness, from reid_profile_get)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine

N_RESIDENT, N_CROPS, ITERS = 1024, 4096, 3


def draw_crops(n, seed=0):
    rng = np.random.default_rng(seed)
    h = np.exp(rng.uniform(np.log(40), np.log(400), n)).astype(np.int64)
    w = np.maximum((h * rng.uniform(0.3, 0.5, n)).astype(np.int64), 1)
    return [rng.integers(0, 256, (int(a), int(b), 3), dtype=np.uint8) for a, b in zip(h, w)]


def timed(fn, sync):
    for _ in range(2):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    sync()
    return (time.perf_counter() - t0) / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = get_engine(0)
    sd = synth.swin_state_dict(0)
    eng.set_precision(0)
    eng.load_swin(*weights.pack_swin(sd)[:2])
    eng.set_precision(2)
    eng.set_chunk(1024)
    out = {"workload": "Swin-T v1, fp32-class (mode 2), 224x224: %d device-resident images against %d ragged uint8 host crops" % (N_RESIDENT, N_CROPS)}

    # the yardstick: device-resident float images, one pass
    x = torch.from_numpy(synth.images_f32(64, 1)).cuda().repeat(N_RESIDENT // 64, 1, 1, 1).contiguous()
    emb = torch.empty((N_RESIDENT, 96), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    el = timed(lambda: eng.swin_embed_dev(x.data_ptr(), N_RESIDENT, 224, 224, emb.data_ptr()), eng.sync)
    resident = N_RESIDENT / el
    out["resident"] = {"images_per_s": round(resident, 1), "ms": round(el * 1e3, 2)}
    del x, emb

    crops = draw_crops(N_CROPS)
    total = sum(c.size for c in crops)
    out["crops"] = {"n": N_CROPS, "bytes": int(total), "mean_bytes": int(total // N_CROPS), "float_image_bytes": 3 * 224 * 224 * 4}
    slab = eng.pinned(total)
    pinned, off = [], 0
    for c in crops:                                   # views of one pinned slab, crop after crop: handed over in place
        v = slab[off:off + c.size].reshape(c.shape)
        v[...] = c
        pinned.append(v)
        off += c.size
    pageable_buf = np.concatenate([c.reshape(-1) for c in crops])
    pageable, off = [], 0
    for c in crops:
        pageable.append(pageable_buf[off:off + c.size].reshape(c.shape))
        off += c.size
    for pipeline in (1, 0):
        eng.debug_switch("host_pipeline", pipeline)
        for name, src in (("pinned", pinned), ("pageable", pageable)):
            el = timed(lambda: eng.swin_embed_ragged_u8(src), eng.sync)
            key = "ragged_%s%s" % (name, "" if pipeline else "_unpipelined")
            out[key] = {"images_per_s": round(N_CROPS / el, 1), "ms": round(el * 1e3, 2), "ratio_to_resident": round(N_CROPS / el / resident, 3),
                        "crop_gb_per_s": round(total / el / 1e9, 2)}
    eng.debug_switch("host_pipeline", 1)

    # the two stems alone, 1024 inputs each
    eng.set_precision(0)
    w, b = np.asarray(sd["sfe.conv1.weight"], np.float32).transpose(0, 2, 3, 1), np.asarray(sd["sfe.conv1.bias"], np.float32)
    sub = crops[:N_RESIDENT]
    pk = np.concatenate([c.reshape(-1) for c in sub])
    offsets = np.concatenate([[0], np.cumsum([c.size for c in sub])[:-1]]).astype(np.int64)
    hw = np.array([c.shape[:2] for c in sub], np.int32)
    xf = np.ascontiguousarray(np.tile(synth.images_f32(64, 1), (N_RESIDENT // 64, 1, 1, 1)))
    kern = {}
    for name, fn in (("swin_crop_front_kernel", lambda: eng.debug_swin_crop_front(pk, offsets, hw, w, b)),
                     ("sfe_conv1_kernel", lambda: eng.debug_swin_conv1(xf, w, b))):
        fn()
        eng.profile(True)
        eng.profile_reset()
        for _ in range(ITERS):
            fn()
        p = eng.profile_get(_ffi.K_ELEMENTWISE)
        eng.profile(False)
        assert p["launches"] == ITERS, p
        kern[name] = {"ms_per_1024": round(p["ms"] / ITERS, 4)}
    out["kernels"] = kern
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
