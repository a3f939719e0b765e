#!/usr/bin/env python3
"""Benchmark of the re-ID embed + match hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Default = the headline alone: set up, W warm-up steps, K timed steps, --dump-outputs if given, ONE JSON line (`value`,
`ms_per_step`, the configuration).  --full = every BASELINE configuration in ONE JSON line: configs[1] is the headline (`value`,
`roofline`, `cpu_baseline` at the top level, the other arithmetic modes as side runs), configs[0]'s batch size / configs[2] /
configs[4] / configs[3] follow as the sub-objects `batch256`, `swin`, `market`, `tracking`, each with its own `roofline` and
bounded `cpu_baseline` (run_all).
Headline = BASELINE configs[1] on every rank: embed 4096 synthetic uint8 crops (128x256, already resident in HBM)
with ResNet18-IBN-SE in fp32-class arithmetic (--precision f16x3, the default: fp32 storage, convolutions as three f16 matrix-core
products per multiply on hi/lo-split operands, fp32 accumulate - held to the exact-fp32 mode's parity bar; with --full the exact-fp32
and the fp16-storage modes are measured in the same run as `f32_path` / `f16_path`), [N>1: ONE RCCL all-gather of the 512-d embeddings, issued through
the C ABI - csrc/comm.hip, no torch.distributed on the data path], then the L2 distance matrix of this rank's 4096
embeddings against all gathered ones.  Weak scaling: per-GPU work is fixed, value = crops of ALL ranks / max-over-ranks
time.  Prints ONE JSON line on rank 0.

One configuration alone, same launch line plus --full --workload (embed = the headline alone, also without --full):
    --workload swin      configs[2]: Swin-T v1, 4096 images 224x224 per rank (weak)
    --workload tracking  configs[3]: 600-frame detection stream, each frame's crops dealt round-robin to the ranks,
                         all-gather of the frame's embeddings, feature-bank cost + DIoU on every rank (strong)
    --workload market    configs[4]: query(3368) x gallery(15913) x 512, gallery rows sharded over the ranks (faiss
                         IndexShards pattern), per-shard top-k, all-gather + device merge, Rank-1 (strong)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = fp32 vector peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # dense f16/bf16 MFMA peak (spec, no sparsity)
PEAK_HBM_GBS = 8000.0
FLOP_PER_CROP = 3.980e9        # 1 990 145 536 MAC
FUSED_BYTES_PER_CROP = 13.78e6 # layer-fused fp32 activation traffic model, SURVEY.md section 8(d)
SWIN_FLOP_PER_IMAGE = 11.54e9  # Swin-T v1 at 224x224


def host_cores():
    """Cores this process may actually use: min(cpu_count, affinity, cgroup CPU quota)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def traffic_from_profile(tag):
    """HBM-side bytes per launch of a kernel class from the committed rocprofv3 PMC passes of this same command
    (tools/pmc_traffic.py: FETCH_SIZE doubled per the gfx950 correction, WRITE_SIZE as is); PMC counters cannot be read
    from inside the process.  The newest profiles/rNN_traffic_<tag>.json wins."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_%s.json" % tag)))
    if not cands:
        return None
    try:
        return round(json.load(open(cands[-1]))["hbm_bytes_per_launch"], 1)
    except (KeyError, ValueError):
        return None


def traffic_source(tag):
    """Where `roofline.traffic` comes from: the committed PMC summary and the commit its library was built from (a constant of
    that profile, not a measurement of this run)."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_%s.json" % tag)))
    if not cands:
        return None
    try:
        return ("profiles/%s (commit %s) - a constant read from that committed PMC profile, not re-measured in this run; a profile of an "
                "earlier round means the kernels of this class have not changed since" % (os.path.basename(cands[-1]), json.load(open(cands[-1])).get("commit", "unknown")))
    except ValueError:
        return None


def sustained_mfma(eng):
    """Registers-only f16 MFMA loops on this device (libreid_hip_debug.so: reid_debug_mfma_bare), TFLOP/s: both instruction shapes,
    random and all-zero operands.  `peak` in the roofline objects stays the nominal figure of MI355X_MICROARCH.md; this is the
    ceiling a kernel with free operands would meet on THIS device, measured in the same process."""
    import ctypes
    if not isinstance(eng.lib, ctypes.CDLL):      # tests/standin_lib.py: no device behind the handle
        return None
    try:
        return {"unit": "TFLOP/s on the f16 pipe, registers only, measured in this run",
                "random_32x32x16": round(eng.debug_mfma_bare(32, False), 1), "random_16x16x32": round(eng.debug_mfma_bare(16, False), 1),
                "zero_32x32x16": round(eng.debug_mfma_bare(32, True), 1), "zero_16x16x32": round(eng.debug_mfma_bare(16, True), 1)}
    except Exception:     # noqa: BLE001 - the debug library is optional
        return None


def cpu_baseline_embed(sd, budget_s=12.0):
    """The oracle (CPU restatement of the reference path) on a bounded sample of the same workload:
    batch 64 (reference default --bs 64), all host cores."""
    import torch
    from oracle import matching, seres18
    from reid_amd import synth
    cores = host_cores()
    torch.set_num_threads(cores)
    crops = synth.crops_u8(64, seed=1)
    seres18.embed_u8(sd, crops)                      # warm-up batch
    n, t0 = 0, time.perf_counter()
    embs = []
    while True:
        embs.append(seres18.embed_u8(sd, crops))
        n += 64
        el = time.perf_counter() - t0
        if el > budget_s or n >= 8192:
            break
    emb = np.concatenate(embs, 0)
    x = np.tile(emb, (max(1, 1024 // emb.shape[0]) + 1, 1))[:1024]
    t1 = time.perf_counter()
    matching.euclidean_dist(x, x)
    dist_ms = (time.perf_counter() - t1) * 1e3
    return {"value": round(n / el, 2), "unit": "crops/s", "cores": cores, "kind": "port",
            "sample": "%d crops (batches of 64, %.1f s) through oracle/seres18.py (torch-CPU restatement, %d threads); "
                      "1024x1024x512 L2 distmat via numpy in %.1f ms" % (n, el, torch.get_num_threads(), dist_ms),
            "distmat_1024_ms": round(dist_ms, 2)}


DUMP_BUDGET_BYTES = 60 * 10**6  # --dump-outputs: array bytes of one run together (under 64 MB with the .npy headers)


def dump_outputs(dirname, outputs):
    """--dump-outputs DIR: what the timed path handed back in its last step, as DIR/<name>.npy (fp32 as is, int32 indices as fp64),
    for comparing two builds output for output.  `outputs` maps a name to a DevArray.  Smallest first, each array gets an equal
    share of what is left of DUMP_BUDGET_BYTES; one larger than its share is written as a fixed sample of its rows
    (numpy default_rng(0), in row order), so the same arguments write the same rows every run."""
    os.makedirs(dirname, exist_ok=True)
    out_dtype = lambda a: np.dtype(np.float32 if a.dtype == np.float32 else np.float64)
    row_bytes = lambda a: int(np.prod(a.shape[1:])) * out_dtype(a).itemsize
    left = DUMP_BUDGET_BYTES
    items = sorted(outputs.items(), key=lambda kv: kv[1].shape[0] * row_bytes(kv[1]))
    for i, (name, arr) in enumerate(items):
        rows = min(arr.shape[0], (left // (len(items) - i)) // row_bytes(arr))
        if rows == arr.shape[0]:
            host = arr.numpy()
        else:
            keep = np.sort(np.random.default_rng(0).choice(arr.shape[0], rows, replace=False))
            host = np.empty((rows,) + arr.shape[1:], arr.dtype)
            for j, r in enumerate(keep):
                arr.engine.d2h(host[j], arr.row_ptr(r))
        host = host.astype(out_dtype(arr))
        np.save(os.path.join(dirname, name + ".npy"), host)
        left -= host.nbytes


class Job:
    """Engine + stream + communicator of this rank, and the timing protocol of the bench contract.  Device, stream and every
    synchronisation go through the C ABI (reid_ctx_create on LOCAL_RANK's device, the context's own non-blocking HIP stream,
    reid_ctx_sync / reid_device_sync); torch is not imported on this path (parallel.RcclComm.from_env uses torch.distributed over
    gloo once, to carry the 128-byte communicator id from rank 0 to the others)."""

    def __init__(self, args):
        from reid_amd import parallel
        from reid_amd.engine import get_engine
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:    # main() launches the ranks itself when WORLD_SIZE is unset; a launcher that disagrees is an error
            print("[bench] FATAL: --gpus %d but WORLD_SIZE=%d" % (args.gpus, self.world), file=sys.stderr, flush=True)
            raise SystemExit(2)
        self.device = self.local_rank      # one rank per device: RCCL rejects two ranks on one GPU ("Duplicate GPU detected")
        if self.world > 1:
            # ONE HIP runtime and ONE librccl per process.  torch.distributed (gloo) carries the communicator id between the ranks,
            # and torch brings its own bundled libamdhip64 / librccl: imported AFTER libreid_hip.so they are loaded beside /opt/rocm's
            # copies and the process aborts in the exit handlers (measured: "double free or corruption", rc -6).  Imported FIRST,
            # libreid_hip.so and its dlopen("librccl.so.1") bind to the copies torch has already loaded - the stack every
            # torch.distributed job on this pool runs on.  A single-rank run never imports torch.
            import torch                    # noqa: F401
            import torch.distributed        # noqa: F401
            # one node (the bench contract): the gloo group that carries the communicator id uses the loopback interface - gloo starts
            # from the hostname, which may not resolve on a pool box (RCCL enumerates interfaces itself and is left alone)
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        self.eng = get_engine(self.device)  # launches + RCCL calls run on the context's own (non-null, non-blocking) HIP stream
        # RCCL communicator behind the C ABI (reid_comm_init) - the only transport: if it cannot be brought up the RCCL error is
        # printed and the job exits non-zero.  REID_BENCH_COMM1=1: a real 1-rank communicator on one GPU
        try:
            self.comm = parallel.RcclComm.from_env(self.eng, single_rank_communicator=os.environ.get("REID_BENCH_COMM1") == "1")
        except Exception as e:     # noqa: BLE001
            print("[bench rank %d] FATAL: RCCL communicator: %s" % (self.rank, e), file=sys.stderr, flush=True)
            raise SystemExit(3)

    def barrier(self):
        self.comm.barrier()                  # RCCL all-reduce of one double + stream sync (local sync when world == 1)
        self.eng.device_sync()               # hipDeviceSynchronize through the C ABI: every stream of this rank's device

    def timed(self, step, steps, warmup):
        """W untimed steps, then EXACTLY `steps` steps bracketed by barrier + synchronize; MAX over ranks."""
        for _ in range(warmup):
            step()
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        self.barrier()
        elapsed = time.perf_counter() - t0
        return float(self.comm.all_reduce([elapsed], "max")[0])

    def close(self):
        self.comm.close()
        # the gloo group RcclComm.from_env made (world > 1).  Only if torch.distributed is ALREADY loaded: importing torch here,
        # after libreid_hip.so has brought in /opt/rocm's HIP runtime and librccl, loads torch's bundled copies of both beside
        # them and the process aborts in the libraries' exit handlers ("double free or corruption", rc -6)
        dist = sys.modules.get("torch.distributed")
        try:
            if dist is not None and dist.is_initialized():
                dist.destroy_process_group()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ configs[1]: embed + distmat
def run_embed(job, args):
    from reid_amd import _ffi, parallel, synth, weights
    eng, comm, world, rank = job.eng, job.comm, job.world, job.rank
    eng.set_chunk(args.chunk)
    sd = synth.seres18_state_dict(0, gem_p=3.0)
    blob, manifest, _ = weights.pack_seres18(sd)
    eng.load_seres18(blob, manifest)

    n, d = args.crops, 512
    # synthetic crops, resident in HBM before the timed region: n DISTINCT crops per rank (BASELINE config 2, seed 1 + rank)
    crops = parallel.DevArray.from_numpy(eng, synth.crops_u8(n, seed=1 + rank))
    emb_all = parallel.DevArray(eng, (n * world, d))
    emb_local = parallel.DevArray(eng, (n, d))
    distmat = parallel.DevArray(eng, (n, n * world))
    lo, hi = parallel.shard_bounds(n * world, world, rank)

    def step():
        # the multi-GPU path of the library itself (parallel.py): embed the local shard, ONE all-gather, row block
        parallel.embed_sharded_dev(eng, comm, crops.ptr, n, n * world, emb_all, emb_local.ptr)
        parallel.distmat_row_block(eng, emb_all, lo, hi, _ffi.METRIC_L2, distmat)

    def run(precision, steps, warmup, dump=None):
        """Timed region per the bench contract; with --full, a profiled repeat of the same steps for the roofline object."""
        eng.set_precision({"f32": 0, "f16": 1, "f16x3": 2}[precision])
        elapsed = job.timed(step, steps, warmup)
        if dump and rank == 0:
            dump_outputs(dump, {"embeddings": emb_all, "distmat": distmat})
        res = {"value": round(n * world * steps / elapsed, 1), "ms_per_step": round(elapsed * 1e3 / steps, 3)}
        if not args.full:
            return res
        # split of one step (embed / all-gather+distmat), HIP events on the launch stream
        eng.timer_start()
        parallel.embed_sharded_dev(eng, comm, crops.ptr, n, n * world, emb_all, emb_local.ptr)
        embed_ms = eng.timer_stop()
        eng.timer_start()
        parallel.distmat_row_block(eng, emb_all, lo, hi, _ffi.METRIC_L2, distmat)
        match_ms = eng.timer_stop()
        # roofline of the dominant kernel class (implicit-GEMM convolutions): the same steps again with every launch
        # of the class bracketed by HIP events on its stream
        eng.profile_reset()
        eng.profile(True)
        tp = time.perf_counter()
        for _ in range(steps):
            step()
        eng.sync()
        prof_ms = (time.perf_counter() - tp) * 1e3 / steps
        conv, dgm, elt = (eng.profile_get(k) for k in (_ffi.K_CONV_GEMM, _ffi.K_DIST_GEMM, _ffi.K_ELEMENTWISE))
        eng.profile(False)
        f16 = precision == "f16"
        x3 = precision == "f16x3"
        # f16x3: every multiply of every convolution is three f16 matrix-core products, so the pipe's dense peak counts a third
        # per ALGORITHMIC flop
        peak = PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F16_MFMA_TFLOPS / 3.0 if x3 else PEAK_F32_MFMA_TFLOPS
        conv_tflops = conv["flops"] / (conv["ms"] * 1e-3) / 1e12 if conv["ms"] > 0 else 0.0
        res.update({
            "embed_ms": round(embed_ms, 3), "embed_crops_per_s_per_gpu": round(n / (embed_ms * 1e-3), 1),
            "distmat_ms": round(match_ms, 3),
            "whole_net_fraction_of_mfma_peak": round(FLOP_PER_CROP * n / (embed_ms * 1e-3) / 1e12 / peak, 4),
            "whole_net_fraction_of_hbm_roofline": round(FUSED_BYTES_PER_CROP * (0.5 if f16 else 1.0) * n / (embed_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
            "roofline": {
                "kernel": ("convolution kernels of the fp16 path, v_mfma_f32_32x32x16_f16: conv3x3_f16 (LDS halo, layers 2-4), conv3x3_c64_f16 (layer 1, weights in registers), stem_pool_f16 (7x7 + BN + maxpool), gemm_f16 (strided / 1x1)" if f16 else
                           "convolution kernels of the fp32-class path, hi/lo-split f16 operands (x.w = xh.wh + (xl.wh + xh.wl), three matrix-core products per multiply, fp32 accumulate; peak = 2.5 PF / 3 per algorithmic flop): conv3x3_x3u (3x3 stride-1: LDS halo, v_mfma_f32_16x16x32_f16, two / three 4-wave blocks per CU, a chunk's 27 steps unrolled; small launches: conv3x3_f16 SPLIT build), conv_x3s (stride-2 3x3 and 1x1: the same block over an im2col gather), stem_split (7x7 + BN + max-pool, v_mfma_f32_32x32x16_f16)" if x3 else
                           "convolution kernels of the fp32 path, v_mfma_f32_32x32x2_f32 (exact fp32): conv_f32_dma_kernel (implicit GEMM, LDS-DMA staging, all 3x3 / 1x1 convs) + the 7x7 stem"),
                "bound": "mfma", "achieved": round(conv_tflops, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(conv_tflops / peak, 4), "traffic": traffic_from_profile("conv_f16" if f16 else "conv_f16x3" if x3 else "conv_f32"),
                "traffic_source": traffic_source("conv_f16" if f16 else "conv_f16x3" if x3 else "conv_f32"),
                "launches": conv["launches"], "avg_launch_us": round(conv["ms"] * 1e3 / max(1, conv["launches"]), 2),
                "algorithmic_gflop_per_launch": round(conv["flops"] / max(1, conv["launches"]) / 1e9, 3),
                "algorithmic_bytes_per_launch": round(conv["bytes"] / max(1, conv["launches"]), 1),
                "profiled_ms_per_step": round(prof_ms, 3),
            },
            "other_kernels": {
                "distmat_gemm": {"ms_per_launch": round(dgm["ms"] / max(1, dgm["launches"]), 3),
                                 "tflops": round(dgm["flops"] / max(dgm["ms"], 1e-9) / 1e9, 2),
                                 "gbs": round(dgm["bytes"] / max(dgm["ms"], 1e-9) / 1e6, 1)},
                "elementwise": {"ms_per_step": round(elt["ms"] / steps, 3),
                                "gbs": round(elt["bytes"] / max(elt["ms"], 1e-9) / 1e6, 1)},
            },
        })
        return res

    main_res = run(args.precision, args.steps, args.warmup, args.dump_outputs)
    arith = {"f32": "exact fp32 (v_mfma_f32_32x32x2_f32), the reference's arithmetic",
             "f16": "fp16 storage, fp32 accumulate (north_star tolerance 1e-3 cosine; measured below)",
             "f16x3": "fp32-class: fp32 storage; every convolution as three f16 matrix-core products per multiply on hi/lo-split "
                      "operands, fp32 accumulate (held to the exact-fp32 mode's parity thresholds in tests/test_gpu_parity.py)"}
    out = {
        "metric": "crops/sec embedded + NxM distmat ms, ResNet18-SE 128x256",
        "value": main_res["value"],
        "unit": "crops/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": main_res["ms_per_step"],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: ResNet18-SE embed %d distinct uint8 crops (128x256) per GPU + %dx%d L2 distmat"
                               % (n, n, n * world),
                   "crops_per_gpu": n, "embed_dim": d, "chunk": args.chunk,
                   "arithmetic": arith[args.precision],
                   "sharding": ("crops sharded by rank, one RCCL all-gather of [N,512] embeddings through the C ABI (reid_allgather_dev)"
                                if world > 1 else "single GPU")},
    }
    if not args.full:                  # a plain run ends here: the side runs, roofline, parity and cpu_baseline are --full's
        return out if rank == 0 else None
    others = {} if args.single else {o: run(o, max(1, min(3, args.steps)), 1) for o in ("f32", "f16x3", "f16") if o != args.precision}
    sustained = sustained_mfma(eng)
    if sustained is not None:
        for res, prec in [(main_res, args.precision)] + [(r, o) for o, r in others.items()]:
            if prec in ("f16", "f16x3"):
                # what the f16 matrix pipe of THIS device sustains on random operands, registers only (the nominal 2.5 PF is not
                # reachable on such data: the chip lowers its clock); the fp32-class kernels of large launches run 16x16x32
                per_flop = sustained["random_16x16x32"] / (3.0 if prec == "f16x3" else 1.0)
                res["roofline"]["sustained_mfma"] = dict(sustained, per_algorithmic_flop=round(per_flop, 1),
                                                         frac_of_sustained=round(res["roofline"]["achieved"] / per_flop, 4))

    # parity inside the bench: the arithmetic modes agree on the embeddings of this rank (cosine against exact fp32)
    e = {}
    for mode, name in ((1, "f16"), (2, "f16x3"), (0, "f32")):
        eng.set_precision(mode)
        eng.embed_u8_dev(crops.ptr, min(256, n), emb_local.ptr)
        e[name] = emb_local.numpy()[:min(256, n)]
    cos = (e["f16"] * e["f32"]).sum(1) / np.linalg.norm(e["f16"], axis=1) / np.linalg.norm(e["f32"], axis=1)
    cos_err = float((1 - cos).max())
    cos3 = (e["f16x3"] * e["f32"]).sum(1) / np.linalg.norm(e["f16x3"], axis=1) / np.linalg.norm(e["f32"], axis=1)
    x3_err = {"max_1_minus_cos": float((1 - cos3).max()), "max_rel_err": float(np.abs(e["f16x3"] - e["f32"]).max() / np.abs(e["f32"]).max())}

    if rank != 0:
        return None
    f16 = args.precision == "f16"
    out["f16_vs_f32_max_cosine_err"] = cos_err
    out["f16x3_vs_f32"] = x3_err
    out.update({k: v for k, v in main_res.items() if k not in ("value", "ms_per_step")})
    for o, r in others.items():
        r["arithmetic"] = arith[o]
        out[o + "_path"] = r
    if not args.no_cpu and world == 1:
        out["cpu_baseline"] = cpu_baseline_embed(sd)
    return out


# ------------------------------------------------------------------------------------------------ configs[2]: Swin-T
def run_swin(job, args):
    from reid_amd import _ffi, parallel, synth, weights
    eng, comm, world, rank = job.eng, job.comm, job.world, job.rank
    n = args.crops
    eng.set_chunk(min(args.chunk, 1024))
    sd = synth.swin_state_dict(0)
    eng.load_swin(*weights.pack_swin(sd)[:2])
    # 256 distinct images per rank repeated (a 4096 x 3 x 224 x 224 fp32 batch is 2.4 GB: generated as 16 x 256)
    base = synth.images_f32(256, 2 + rank)
    x = parallel.DevArray(eng, (n, 3, 224, 224))
    for i in range(0, n, 256):
        m = min(256, n - i)
        eng.h2d(x.row_ptr(i), base[:m])
    emb_local = parallel.DevArray(eng, (n, 96))
    emb_all = parallel.DevArray(eng, (n * world, 96))

    def step():
        eng.swin_embed_dev(x.ptr, n, 224, 224, emb_local.ptr)
        comm.all_gather(emb_local.ptr, emb_all.ptr, n * 96 * 4)

    def run(precision, steps, warmup, dump=None):
        eng.set_precision({"f32": 0, "f16": 1, "f16x3": 2}[precision])
        elapsed = job.timed(step, steps, warmup)
        if dump and rank == 0:
            dump_outputs(dump, {"embeddings": emb_all})
        eng.profile_reset()
        eng.profile(True)
        for _ in range(steps):
            step()
        eng.sync()
        g, e = eng.profile_get(_ffi.K_CONV_GEMM), eng.profile_get(_ffi.K_ELEMENTWISE)
        eng.profile(False)
        f16 = precision == "f16"
        x3 = precision == "f16x3"   # three f16 matrix-core products per algorithmic multiply: a third of the pipe's dense peak
        peak = PEAK_F16_MFMA_TFLOPS if f16 else PEAK_F16_MFMA_TFLOPS / 3.0 if x3 else PEAK_F32_MFMA_TFLOPS
        tf = g["flops"] / max(g["ms"], 1e-9) / 1e9
        return {"value": round(n * world * steps / elapsed, 1), "ms_per_step": round(elapsed * 1e3 / steps, 3),
                "whole_net_tflops": round(SWIN_FLOP_PER_IMAGE * n * steps / elapsed / 1e12, 1),
                # exact fp32: the contractions are bound by the fp32 MFMA rate; fp16 storage: by HBM (PMC traffic of the class
                # ~3.7 TB/s at its average launch duration, profiles/r02_traffic_swin_f16.json) - algorithmic bytes / duration
                "roofline": ({"kernel": "Swin Linear / conv contractions (gemm_f16 linear builds, v_mfma_f32_32x32x16_f16)",
                              "bound": "hbm", "achieved": round(g["bytes"] / max(g["ms"], 1e-9) / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": round(g["bytes"] / max(g["ms"], 1e-9) / 1e6 / PEAK_HBM_GBS, 4),
                              "traffic": traffic_from_profile("swin_f16"), "launches": g["launches"],
                              "avg_launch_us": round(g["ms"] * 1e3 / max(1, g["launches"]), 2),
                              "algorithmic_bytes_per_launch": round(g["bytes"] / max(1, g["launches"]), 1),
                              "mfma_tflops": round(tf, 2), "mfma_frac": round(tf / peak, 4)} if f16 else
                             {"kernel": ("Swin Linear / conv contractions, fp32-class (stages 1-2: fused pairs of linears and LayerNorm + "
                                         "to_qkv of two_linear_f16.hip; stages 3-4: lin_x3_kernel - 4-wave blocks, two per CU, v_mfma_f32_16x16x32_f16; "
                                         "the trunk convolutions: gemm_f16 linear builds; hi/lo-split operands, three f16 MFMA products "
                                         "per multiply; peak = f16 dense / 3)" if x3 else
                                         "Swin Linear / conv contractions (gemm_f32_dma / conv_f32_dma, v_mfma_f32_32x32x2_f32)"),
                              "bound": "mfma", "achieved": round(tf, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                              "traffic": traffic_from_profile("swin_f16x3" if x3 else "swin_f32"), "launches": g["launches"],
                              "avg_launch_us": round(g["ms"] * 1e3 / max(1, g["launches"]), 2),
                              "algorithmic_bytes_per_launch": round(g["bytes"] / max(1, g["launches"]), 1)}),
                "other_kernels": {"elementwise_attention_norm": {"ms_per_step": round(e["ms"] / steps, 3)}}}

    main_prec = args.precision
    main_res = run(main_prec, args.steps, args.warmup, args.dump_outputs)
    # what was timed is checked before it is printed: the embeddings of the timed configuration (passes of up to 1024 images) are
    # finite, and six of them agree with the exact-fp32 mode's on the same images (images are independent,
    # swin_transformer.py:191-232,248-260; the GPU tests hold exact fp32 to the reference's vectors)
    eng.set_precision({"f32": 0, "f16": 1, "f16x3": 2}[main_prec])
    step()
    got = emb_local.numpy()
    if not np.isfinite(got).all():
        raise RuntimeError("swin: non-finite embeddings in the timed configuration")
    eng.set_precision(0)
    six = parallel.DevArray(eng, (6, 96))
    eng.swin_embed_dev(x.ptr, 6, 224, 224, six.ptr)
    want = six.numpy()
    cos6 = (got[:6] * want).sum(1) / np.linalg.norm(got[:6], axis=1) / np.linalg.norm(want, axis=1)
    check = {"rows": 6, "max_1_minus_cos_vs_exact_fp32": float((1 - cos6).max()),
             "max_rel_err_vs_exact_fp32": float(np.abs(got[:6] - want).max() / np.abs(want).max())}
    if check["max_1_minus_cos_vs_exact_fp32"] > (1e-4 if main_prec == "f16" else 1e-5):
        raise RuntimeError("swin: timed configuration disagrees with exact fp32: %r" % (check,))
    others = {} if args.single else {o: run(o, max(1, min(2, args.steps)), 1) for o in ("f32", "f16x3", "f16") if o != main_prec}
    if rank != 0:
        return None
    out = {"metric": "images/sec embedded, Swin-T v1 224x224", "value": main_res["value"], "unit": "images/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": main_res["ms_per_step"], "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": main_prec, "data": "synthetic",
           "config": {"workload": "BASELINE configs[2]: Swin-T v1 backbone, %d images 224x224 per GPU (+ all-gather of the 96-d embeddings)" % n,
                      "images_per_gpu": n, "embed_dim": 96, "chunk": min(args.chunk, 1024)}}
    out.update({k: v for k, v in main_res.items() if k not in ("value", "ms_per_step")})
    out["self_check"] = check
    for o, r in others.items():
        out[o + "_path"] = r
    if not args.no_cpu and world == 1:
        import torch
        from oracle import swin
        cores = host_cores()
        torch.set_num_threads(cores)
        xs = base[:16]
        swin.embed(sd, xs)
        t0, m = time.perf_counter(), 0
        while time.perf_counter() - t0 < 10:
            swin.embed(sd, xs)
            m += 16
        el = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(m / el, 2), "unit": "images/s", "cores": cores, "kind": "port",
                               "sample": "%d images (batches of 16, %.1f s) through oracle/swin.py (torch-CPU restatement)" % (m, el)}
    return out


# ------------------------------------------------------------------------------------------------ configs[3]: tracking stream
TRACK_WARMUP = 60   # untimed frames: workspaces and pinned staging reach the sizes of the stream's larger frames


def run_tracking(job, args):
    """MOT16-02 is not in the container: synthetic stand-in per SURVEY.md section 8(d) - 600 frames, detections per frame
    ~ Poisson(30) clipped to [1, 80], ragged crop sizes.  Per frame: this rank's share of the crops (round-robin) is resized
    and embedded on the device, ONE all-gather of the frame's embeddings, then - on every rank, as DeepSORT would -
    the feature-bank cost against 40 tracks x 100 samples (gated at MAX_DIST 0.15) and the DIoU cost."""
    from reid_amd import parallel, synth, weights
    from reid_amd.iou_matching import iou_cost
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    eng, comm, world, rank = job.eng, job.comm, job.world, job.rank
    sd = synth.seres18_state_dict(0, gem_p=3.0)
    eng.load_seres18(*weights.pack_seres18(sd)[:2])
    eng.set_precision({"f32": 0, "f16": 1, "f16x3": 2}[args.precision])
    frames = args.frames
    rng = np.random.default_rng(3)
    counts = np.clip(rng.poisson(30, frames), 1, 80)
    pool = synth.ragged_crops_u8(256, seed=3)
    from reid_amd.tracking import ShardedCameraStream
    # MAX_DIST / NN_BUDGET, deep_sort.yaml:3,9.  The match stream only where no collective runs (tracking.ShardedCameraStream: beside
    # librccl's streams it costs more than half the rate); --match-stream 2 forces it for that A/B
    two = args.match_stream == 2 or (bool(args.match_stream) and world == 1 and not getattr(comm, "active", False))
    stream = ShardedCameraStream(eng, comm, 0.15, 100, match_stream=two)
    metric = stream.metric
    tracks = list(range(40))
    metric.partial_fit(rng.normal(size=(40 * 100, 512)).astype(np.float32), np.repeat(tracks, 100), tracks)
    boxes = rng.uniform(0, 500, (80, 4))
    boxes[:, 2:] = rng.uniform(20, 120, (80, 2))
    per_max = (80 + world - 1) // world
    d_local = parallel.DevArray(eng, (per_max, 512))
    d_all = parallel.DevArray(eng, (per_max * world, 512))
    gather_us = []

    def frame(f, timed=False):
        n = int(counts[f])
        mine = parallel.round_robin(n, world, rank)
        crops = [pool[(f * 7 + int(i)) % 256] for i in mine]
        local = eng.embed_ragged_u8(crops) if len(crops) else np.empty((0, 512), np.float32)
        if world > 1:
            # equal-size slots (ceil(n / world) rows, zero padded): one ncclAllGather, no count exchange
            per = (n + world - 1) // world
            buf = np.zeros((per, 512), np.float32)
            buf[: len(local)] = local
            eng.h2d(d_local.ptr, buf)
            t0 = time.perf_counter()
            comm.all_gather(d_local.ptr, d_all.ptr, per * 512 * 4)
            eng.sync()
            if timed:
                gather_us.append((time.perf_counter() - t0) * 1e6)
            allb = np.empty((world * per, 512), np.float32)
            eng.d2h(allb, d_all.ptr)
            feats = np.empty((n, 512), np.float32)
            for r in range(world):
                idx = parallel.round_robin(n, world, r)
                feats[idx] = allb[r * per: r * per + len(idx)]
        else:
            feats = local
        cost = metric.distance(feats, tracks, max_distance=0.15)
        icost = iou_cost(boxes[:40], boxes[:n])
        k = min(n, 40)
        metric.partial_fit(feats[:k], tracks[:k], tracks)
        return n, cost, icost

    def crops_of(f):
        return [pool[(f * 7 + i) % 256] for i in range(int(counts[f]))]

    def run_pipelined(first, last, lat):
        """The frame pipeline (csrc/bank.hip) through the library's own driver, tracking.ShardedCameraStream, for any number of
        ranks: this rank's round-robin share of frame f+1 is packed into pinned memory, uploaded and embedded while frame f's
        costs come back and its update is enqueued; the ranks' embeddings meet in ONE device-side all-gather per frame
        (reid_frame_gather), every rank then holds the frame's features in the slot and computes the full cost matrices, as
        DeepSORT would on every rank.  One wait per frame."""
        stream.submit(crops_of(first))
        t_sub = {first: time.perf_counter()}
        total = 0
        for f in range(first, last):
            n = int(counts[f])
            nxt = crops_of(f + 1) if f + 1 < last else None
            t0 = time.perf_counter()
            if nxt is not None:
                t_sub[f + 1] = t0
            feats, cost, icost = stream.step(n, tracks, boxes[:40], boxes[:n], nxt)
            if world > 1:
                gather_us.append((time.perf_counter() - t0) * 1e6)              # gather + costs + the frame's wait
            k = min(n, 40)
            stream.commit(np.arange(k), tracks[:k], tracks)
            lat.append(time.perf_counter() - t_sub.pop(f))
            total += n
        eng.sync()
        return total

    pipelined = not args.no_pipeline
    if pipelined:
        run_pipelined(0, TRACK_WARMUP, [])
    else:
        for f in range(TRACK_WARMUP):
            frame(f)
    job.barrier()
    t0 = time.perf_counter()
    ncrops = 0
    lat = []
    if pipelined:
        ncrops = run_pipelined(0, frames, lat)
    else:
        for f in range(frames):
            t1 = time.perf_counter()
            ncrops += frame(f, timed=True)[0]
            lat.append(time.perf_counter() - t1)
    job.barrier()
    elapsed = float(comm.all_reduce([time.perf_counter() - t0], "max")[0])
    # roofline object of the frame's convolutions: the first 100 frames again with every launch of the class bracketed by HIP
    # events on its stream (same flow as the timed region; on EVERY rank - the frames hold a collective)
    from reid_amd import _ffi
    eng.profile_reset()
    eng.profile(True)
    nprof = min(100, frames)
    if pipelined:
        run_pipelined(0, nprof, [])
    else:
        for f in range(nprof):
            frame(f)
    eng.sync()
    conv = eng.profile_get(_ffi.K_CONV_GEMM)
    eng.profile(False)
    job.barrier()
    if not (pipelined and world == 1 and args.cameras > 1):
        stream.metric.close()
        eng.set_precision(0)
    if rank != 0:
        return None
    lat = np.asarray(lat) * 1e3
    cpu = None
    if not args.no_cpu and world == 1:
        # the oracle on the same stream, bounded: preprocess (cv2-style resize) + ResNet18-SE on the CPU + numpy cosine cost + DIoU
        import torch
        from oracle import matching, seres18
        cores = host_cores()
        torch.set_num_threads(cores)
        bank = rng.normal(size=(40, 100, 512)).astype(np.float32)
        bank /= np.linalg.norm(bank, axis=2, keepdims=True)
        t0c, fc, cc = time.perf_counter(), 0, 0
        while time.perf_counter() - t0c < 10.0 and fc < frames:
            nf = int(counts[fc])
            cr = [pool[(fc * 7 + i) % 256] for i in range(nf)]
            e, _ = seres18.forward(sd, torch.from_numpy(matching.preprocess(cr)))
            e = e.numpy()
            e /= np.linalg.norm(e, axis=1, keepdims=True)
            (1.0 - np.einsum("tbd,md->tbm", bank, e)).min(1)                 # _nn_cosine_distance per track
            matching.diou_cost(boxes[:40], boxes[:nf])
            fc += 1
            cc += nf
        elc = time.perf_counter() - t0c
        cpu = {"value": round(fc / elc, 2), "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "%d frames, %d crops (%.1f s): oracle preprocess + oracle/seres18.py + numpy bank cost + DIoU" % (fc, cc, elc)}
    peak = {"f16": PEAK_F16_MFMA_TFLOPS, "f16x3": PEAK_F16_MFMA_TFLOPS / 3.0, "f32": PEAK_F32_MFMA_TFLOPS}[args.precision]
    conv_tf = conv["flops"] / (conv["ms"] * 1e-3) / 1e12 if conv["ms"] > 0 else 0.0
    roof = {"kernel": "convolution kernels of a frame's forward (~%d crops per rank: launches of at most one wave of blocks, latency-bound K loops)"
                      % round(ncrops / frames / world),
            "bound": "mfma", "achieved": round(conv_tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(conv_tf / peak, 4), "traffic": None,
            "launches": conv["launches"], "avg_launch_us": round(conv["ms"] * 1e3 / max(1, conv["launches"]), 2),
            "conv_ms_per_frame": round(conv["ms"] / nprof, 4)}
    multi = None
    if pipelined and world == 1 and args.cameras > 1:
        # several camera streams on the one GPU: own context (HIP stream, workspaces, bank) and host thread each
        import threading
        from reid_amd.tracking import CameraStream
        blob, manifest = weights.pack_seres18(sd)[:2]
        def drive(cs, c, first, last):
            cr = lambda f: [pool[(f * 7 + i + 31 * c) % 256] for i in range(int(counts[f]))]
            cs.submit(cr(first))
            for f in range(first, last):
                n = int(counts[f])
                cs.step(tracks, boxes[:40], boxes[:n], cr(f + 1) if f + 1 < last else None)
                k = min(n, 40)
                cs.commit(np.arange(k), tracks[:k], tracks)
            cs.close()

        def threads_form(two_streams):
            cams = []
            for c in range(args.cameras):
                cs = CameraStream(blob, manifest, {"f32": 0, "f16": 1, "f16x3": 2}[args.precision], match_stream=two_streams)
                cs.metric.partial_fit(rng.normal(size=(40 * 100, 512)).astype(np.float32), np.repeat(tracks, 100), tracks)
                cams.append(cs)
            for c, cs in enumerate(cams):
                drive(cs, c, 0, 40)
            th = [threading.Thread(target=drive, args=(cs, c, 0, frames)) for c, cs in enumerate(cams)]
            t0m = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            el = time.perf_counter() - t0m
            for cs in cams:
                cs.close(destroy=True)
            return el
        # K contexts as in rounds 2-5: everything of a camera on its one compute stream; and with each camera's cost / update stages on
        # a second, high-priority stream (the default of a single CameraStream: with K contexts it is 2K + K copy streams on the device's
        # few hardware queues, and the cross-stream waits stall on queue switches)
        elm, elm2 = threads_form(False), threads_form(True)
        # the same K cameras batched into ONE pass per frame time (tracking.MultiCameraStream: one context, one host thread, per-camera
        # banks and per-camera cost blocks) - the mapping that pays: a pass of ~30 K crops runs its convolutions as proper tiles
        from reid_amd.tracking import MultiCameraStream
        K = args.cameras
        mc = MultiCameraStream(blob, manifest, K, {"f32": 0, "f16": 1, "f16x3": 2}[args.precision])
        for met in mc.metrics:
            met.partial_fit(rng.normal(size=(40 * 100, 512)).astype(np.float32), np.repeat(tracks, 100), tracks)

        def crk(f):
            return [[pool[(f * 7 + i + 31 * c) % 256] for i in range(int(counts[f]))] for c in range(K)]

        def drive_batched(first, last):
            mc.submit(crk(first))
            for f in range(first, last):
                n = int(counts[f])
                mc.step([tracks] * K, [boxes[:40]] * K, [boxes[:n]] * K, crk(f + 1) if f + 1 < last else None)
                k = min(n, 40)
                mc.commit([np.arange(k)] * K, [tracks[:k]] * K, [tracks] * K)
            mc.eng.sync()
        drive_batched(0, 40)
        t0b = time.perf_counter()
        drive_batched(0, frames)
        elb = time.perf_counter() - t0b
        mc.close(destroy=True)
        multi = {"cameras": K, "frames_per_s_total": round(K * frames / elb, 1),
                 "frames_per_s_per_camera": round(frames / elb, 1), "ms_per_frame_time": round(elb / frames * 1e3, 3),
                 "mode": "batched: the K cameras' crops of a frame time in ONE pass (tracking.MultiCameraStream), per-camera banks and cost blocks, one host thread",
                 "threads": {"frames_per_s_total": round(K * frames / elm, 1), "frames_per_s_per_camera": round(frames / elm, 1),
                             "ms_per_frame_per_camera": round(elm / frames * 1e3, 3),
                             "mode": "K contexts, K host threads, one pass per camera frame, match_stream=False (rounds 2-5)",
                             "frames_per_s_total_with_match_streams": round(K * frames / elm2, 1)}}
    out = {"metric": "frames/sec, per-frame crop batches embedded + gathered + matched (ResNet18-SE 128x256)", "value": round(frames / elapsed, 1),
            "unit": "frames/s", "n_gpus": world, "steps": frames, "warmup": TRACK_WARMUP, "ms_per_step": round(elapsed * 1e3 / frames, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": "BASELINE configs[3] stand-in: %d frames, %d crops (Poisson(30) per frame, ragged sizes), round-robin over "
                                   "the ranks, all-gather of [n_f,512], bank cost (40 tracks x 100) + DIoU" % (frames, ncrops),
                       "host_flow": ("frame pipeline: " + ("device all-gather f | " if world > 1 else "") + "cost f | submit f+1 | fetch f (the one wait) | update f")
                                    if pipelined else "one synchronous call per operation"},
            "crops_per_s": round(ncrops / elapsed, 1), "ms_per_frame_median": round(float(np.median(lat)), 3),
            "ms_per_frame_p95": round(float(np.percentile(lat, 95)), 3),
            "allgather_us_median": round(float(np.median(gather_us)), 1) if gather_us else None}
    out["roofline"] = roof
    if pipelined and world == 1 and args.cameras > 1:
        # the same stream when detections are known ahead (a video file, this detection dump): F consecutive frames embedded as ONE
        # pass, costs and bank updates per frame and in order (tracking.LookaheadCameraStream).  Throughput form - a frame's features
        # wait for the F-th frame of its group; `value` above stays the strict frame-by-frame stream.
        from reid_amd.tracking import LookaheadCameraStream
        blob, manifest = weights.pack_seres18(sd)[:2]
        look = {}
        for F in (2, 4):
            la = LookaheadCameraStream(blob, manifest, F, {"f32": 0, "f16": 1, "f16x3": 2}[args.precision])
            la.metric.partial_fit(rng.normal(size=(40 * 100, 512)).astype(np.float32), np.repeat(tracks, 100), tracks)

            def drive_la(first, last):
                grp = lambda g0: [crops_of(f) for f in range(g0, min(g0 + F, last))]
                la.submit_group(grp(first))
                for g0 in range(first, last, F):
                    for j, f in enumerate(range(g0, min(g0 + F, last))):
                        n = int(counts[f])
                        ts = time.perf_counter()
                        la.step(j, tracks, boxes[:40], boxes[:n], grp(g0 + F) if (j == la.handover and g0 + F < last) else None)
                        step_s[j].append(time.perf_counter() - ts)
                        k = min(n, 40)
                        la.commit(j, np.arange(k), tracks[:k], tracks)
                la.eng.sync()
            step_s = [[] for _ in range(F)]
            drive_la(0, 40)
            step_s = [[] for _ in range(F)]
            t0l = time.perf_counter()
            drive_la(0, frames)
            ell = time.perf_counter() - t0l
            la.close(destroy=True)
            look["frames_per_pass_%d" % F] = {"frames_per_s": round(frames / ell, 1), "ms_per_frame": round(ell / frames * 1e3, 3),
                                              "step_ms_by_frame_of_group": [round(float(np.mean(v)) * 1e3, 3) for v in step_s]}
        look["note"] = ("detections known F frames ahead (video file / detection dump): F frames' crops in one pass, costs and bank updates per frame "
                        "in order on a stream of their own beside the next group's forward; latency = F frame periods.  Not `value`.")
        out["lookahead"] = look
    if multi is not None:
        stream.metric.close()
        eng.set_precision(0)
        out["camera_streams"] = multi
    if cpu is not None:
        out["cpu_baseline"] = cpu
    eng.frame_match_stream(False)
    return out


# ------------------------------------------------------------------------------------------------ configs[4]: Market-sized retrieval
def run_market(job, args):
    from reid_amd import _ffi, parallel, synth
    eng, comm, world, rank = job.eng, job.comm, job.world, job.rank
    nq, ng, d, k = 3368, 15913, 512, 20
    qf, ql, qc, gf, gl, gc = synth.clustered_embeddings(nq, ng, d=d, n_ids=751, n_cams=6, seed=4, sigma=3.0)
    lo, hi = parallel.shard_bounds(ng, world, rank)
    dq = parallel.DevArray.from_numpy(eng, qf)
    dg = parallel.DevArray.from_numpy(eng, gf[lo:hi])                   # this rank's gallery rows only
    dist = parallel.DevArray(eng, (nq, max(hi - lo, 1)))
    dD, dI = parallel.DevArray(eng, (nq, k)), parallel.DevArray(eng, (nq, k), np.int32)

    def step():
        # the shard's block of the distance matrix (the metric's "N x M distmat ms") + sharded k-NN with device merge
        if hi > lo:
            eng.distmat_dev(dq.ptr, nq, dg.ptr, hi - lo, d, _ffi.METRIC_L2, dist.ptr)
        parallel.knn_gallery_sharded_dev(eng, dq.ptr, nq, dg.ptr, hi - lo, lo, d, k, dD.ptr, dI.ptr, world)

    elapsed = job.timed(step, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"distmat": dist, "knn_dist": dD, "knn_index": dI})
    eng.timer_start()
    if hi > lo:
        eng.distmat_dev(dq.ptr, nq, dg.ptr, hi - lo, d, _ffi.METRIC_L2, dist.ptr)
    dist_ms = eng.timer_stop()
    eng.timer_start()
    for _ in range(5):       # the search alone: fused distance + top-20 (no matrix) + exchange + merge
        parallel.knn_gallery_sharded_dev(eng, dq.ptr, nq, dg.ptr, hi - lo, lo, d, k, dD.ptr, dI.ptr, world)
    search_ms = eng.timer_stop() / 5
    I = dI.numpy()
    # Rank-1 over the merged lists, reference rule (reid/evaluate.py:55-105): first item that is not junk (same id AND same camera)
    junk = (gl[I] == ql[:, None]) & (gc[I] == qc[:, None])
    first = np.where(junk, I.shape[1], np.arange(I.shape[1])[None, :]).min(1)
    ok = first < I.shape[1]
    rank1 = float((gl[I[np.arange(nq), np.minimum(first, I.shape[1] - 1)]] == ql)[ok].sum() / nq)
    if rank != 0:
        return None
    flops = 2.0 * nq * (hi - lo) * d
    byts = 4.0 * (nq * d + (hi - lo) * d + nq * (hi - lo))
    out = {"metric": "N x M distmat ms + rank-1, query(3368) x gallery(15913) x 512", "value": round(nq * args.steps / elapsed, 1),
           "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed * 1e3 / args.steps, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "BASELINE configs[4]: 3368 x 15913 x 512, gallery rows sharded over %d rank(s): shard distance matrix, then "
                                  "the search - top-%d per shard: candidates from an fp32-class GEMM on the f16 matrix pipe, exact fp32 "
                                  "refinement (knn_wide.hip: the numbers and order of the fused fp32 search, which shards below 2^25 pairs "
                                  "still take), all-gather (fp32 distances, int32 indices), device k-way merge" % (world, k)},
           "distmat_shard_ms": round(dist_ms, 3), "search_ms": round(search_ms, 3),
           "search_tflops": round(2.0 * nq * (hi - lo) * d / (search_ms * 1e-3) / 1e12, 2), "rank1_top%d" % k: rank1,
           "roofline": {"kernel": "gemm_f32_dma_kernel<E_DIST> (dense LDS-DMA GEMM + distance epilogue, v_mfma_f32_32x32x2_f32)", "bound": "mfma",
                        "achieved": round(flops / (dist_ms * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(flops / (dist_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "traffic": traffic_from_profile("market"),
                        "algorithmic_bytes_per_launch": byts, "hbm_gbs": round(byts / (dist_ms * 1e-3) / 1e9, 1)}}
    if not args.no_cpu and world == 1:
        from oracle import matching
        t0 = time.perf_counter()
        matching.euclidean_dist(qf[:1024], gf)
        el = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(1024 / el, 1), "unit": "queries/s", "cores": host_cores(), "kind": "port",
                               "sample": "1024 x 15913 x 512 L2 distance matrix through oracle/matching.py (numpy) in %.1f ms" % (el * 1e3)}
    return out


SUB_KEYS = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "scaling", "dtype", "config", "roofline", "cpu_baseline",
            "f16_path", "f32_path", "f16x3_path", "f16x3_vs_f32", "other_kernels", "embed_ms", "distmat_ms", "distmat_shard_ms", "search_ms", "search_tflops",
            "crops_per_s", "ms_per_frame_median", "ms_per_frame_p95", "allgather_us_median", "camera_streams", "lookahead", "rank1_top20",
            "whole_net_tflops", "f16_vs_f32_max_cosine_err", "self_check", "plugin_default")


def run_all(job, args):
    """The --full line: BASELINE configs[1] as the headline (value / roofline / cpu_baseline as before) plus the other
    configurations as sub-objects of the SAME JSON line, each with its own roofline and bounded cpu_baseline:
    `batch256` (configs[0]'s size: 256 crops + 256 x 256 distmat), `swin` (configs[2]), `market` (configs[4]), `tracking`
    (configs[3] stand-in, exact fp32 with the fp16-storage run nested as f16_path).  A sub-workload that raises is reported as
    {"error": ...}; one that does not come back within its time limit (a collective some rank never entered) ends the job
    from a watchdog thread: rank 0 prints the line with what it has and EVERY rank leaves with a non-zero exit code (3), so the
    launcher and the driver see the failure.  REID_BENCH_LIMIT_SCALE scales the time limits (tests)."""
    import copy
    import tempfile
    import threading
    state = {"out": None, "current": None, "deadline": None}
    # "rank 0 has printed the line": a flag file named after this job's rendezvous.  Every rank's watchdog fires on its own clock,
    # and the launcher (torch.distributed.run) SIGTERMs the remaining ranks as soon as ONE exits non-zero - so a rank other than 0
    # must not leave before rank 0 has written what it has (it waits for the flag, bounded), or the partial line is lost.
    flag = os.path.join(tempfile.gettempdir(), "reid_bench_%s_%s_%s.emitted" % (
        os.environ.get("MASTER_ADDR", "local"), os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", str(os.getppid()))))
    if job.rank == 0:
        try:
            os.unlink(flag)
        except OSError:
            pass

    def leave_failed(line_out):
        """Rank 0: print the partial line, raise the flag, exit 3.  Other ranks: wait until the flag is up (at most 10 s), exit 3."""
        if job.rank == 0:
            if line_out is not None:
                emit(json.dumps(line_out))
            try:
                open(flag, "w").close()
            except OSError:
                pass
            import atexit
            atexit.register(lambda: os.path.exists(flag) and os.unlink(flag))   # (os._exit below skips it: the next job of this rendezvous unlinks a stale flag)
        elif job.world > 1:
            # rank 0's watchdog runs on the same limit from its own clock: wait for what is left of the current sub-workload's limit plus a
            # margin, not a fixed 10 s (an exception on this rank can come long before rank 0's deadline)
            left = (state["deadline"] - time.monotonic()) if state["deadline"] is not None else 0.0
            t_end = time.monotonic() + max(10.0, left + 15.0)
            while not os.path.exists(flag) and time.monotonic() < t_end:
                time.sleep(0.05)
        os._exit(3)                           # a lost collective / hung or failed sub-workload is a FAILED run

    def watchdog():
        while True:
            time.sleep(0.25)
            dl = state["deadline"]
            if dl is not None and job.rank == 0:       # tests: force the order "another rank notices first" (seconds added to rank 0's limit)
                dl += float(os.environ.get("REID_BENCH_TEST_RANK0_WATCHDOG_DELAY", "0"))
            if dl is not None and time.monotonic() > dl:
                print("[bench rank %d] watchdog: %s did not come back within its time limit" % (job.rank, state["current"]),
                      file=sys.stderr, flush=True)
                if job.rank == 0 and state["out"] is not None:
                    state["out"][state["current"]] = {"error": "no answer within the time limit (watchdog)"}
                leave_failed(state["out"])

    out = run_embed(job, args)
    state["out"] = out
    threading.Thread(target=watchdog, daemon=True).start()

    def sub(name, fn, limit_s, **over):
        a = copy.copy(args)
        a.dump_outputs = None                 # --dump-outputs: the headline's timed path only
        for k, v in over.items():
            setattr(a, k, v)
        state["current"], state["deadline"] = name, time.monotonic() + limit_s * float(os.environ.get("REID_BENCH_LIMIT_SCALE", "1"))
        try:
            res = fn(job, a)
            if res is not None:
                res = {k: res[k] for k in SUB_KEYS if k in res}
        except Exception as e:     # noqa: BLE001 - recorded in the line; the remaining sub-workloads still run on one GPU
            res = {"error": "%s: %s" % (type(e).__name__, e)}
            if job.world > 1:      # the ranks are no longer in step: stop here (the watchdog releases ranks stuck in a collective)
                state["deadline"] = time.monotonic() + 20
                if out is not None:
                    out[name] = res
                raise
        state["deadline"] = None
        if out is not None:
            out[name] = res

    def tracking_both(job_, a):
        r32 = run_tracking(job_, a)
        for prec in [q for q in ("f16x3", "f32", "f16") if q != a.precision]:
            a2 = copy.copy(a)
            a2.precision, a2.no_cpu, a2.cameras = prec, True, 0      # (camera groups / look-ahead: the headline arithmetic only - run time)
            r2 = run_tracking(job_, a2)
            if r32 is not None:
                r32[prec + "_path"] = {k: r2[k] for k in ("value", "ms_per_step", "crops_per_s", "ms_per_frame_median", "ms_per_frame_p95",
                                                           "roofline", "camera_streams", "lookahead") if k in r2}
        return r32

    try:
        sub("batch256", run_embed, 240, crops=256, steps=20, warmup=3, no_cpu=True)
        sub("swin", run_swin, 300, crops=4096, steps=2, warmup=1)
        sub("market", run_market, 240, steps=20, warmup=3)
        sub("tracking", tracking_both, 300, cameras=4 if job.world == 1 else 0)
    except Exception as e:     # noqa: BLE001 - multi-rank job out of step: print what there is and leave
        print("[bench rank %d] sub-workload failed: %r" % (job.rank, e), file=sys.stderr, flush=True)
        state["deadline"] = None              # this thread prints and leaves; the watchdog must not race it
        leave_failed(out)                     # ranks out of step: never report success
    state["deadline"] = None
    if out is not None:
        out["plugin_default"] = plugin_default(job, out)
        if job.world == 1:
            out["host_path"] = host_path(job, out, args)
    return out


def plugin_default(job, out):
    """What the drop-in surface delivers when the tracker sets nothing: the arithmetic Extractor / build_model pick by default
    (reid_amd.precision: $REID_PRECISION, else f16x3), this line's numbers for THAT arithmetic by name, and the synchronous
    plugin call itself - Extractor.__call__ on ~30 ragged crops, packed, uploaded, resized, embedded and downloaded per call, as
    track_yolov5.py:178-253 drives it (feature_extractor.py:48-53)."""
    from reid_amd import precision, synth
    from reid_amd.extractor import Extractor
    label = precision.LABEL[precision.resolve(None)]

    def pick(obj):
        if not isinstance(obj, dict):
            return None
        return obj if obj.get("dtype") == label else obj.get(label + "_path")
    head, trk = pick(out), pick(out.get("tracking"))
    res = {"precision": label,
           "crops_per_s": head.get("value") if head else None,
           "tracking_frames_per_s": trk.get("value") if trk else None}
    try:
        ext = Extractor(synth.seres18_state_dict(0, gem_p=3.0))
        pool = synth.ragged_crops_u8(256, seed=3)
        frames = [[pool[(f * 7 + i) % 256] for i in range(30)] for f in range(40)]
        for fr in frames[:10]:
            ext(fr)
        t0 = time.perf_counter()
        for _ in range(5):
            for fr in frames:
                ext(fr)
        el = time.perf_counter() - t0
        res["extractor_call_30_crops_ms"] = round(el / 200 * 1e3, 3)
        res["extractor_calls_per_s"] = round(200 / el, 1)
        res["extractor_precision_after"] = ext.precision
    except Exception as e:     # noqa: BLE001
        res["error"] = "%s: %s" % (type(e).__name__, e)
    return res


def host_path(job, out, args):
    """The path the reference actually has - host crops in, host features out (feature_extractor.py:48-53: `.to(device)` ...
    `.cpu().numpy()`; image_reid_inference.py:116-122 per batch): `Extractor(crops)` of the drop-in surface on 256 and on `--crops`
    host crops, PCIe transfers INSIDE the timed calls.  Never `value` (the bench contract times device-resident inputs); reported
    beside it as crops/s and as a fraction of `value`.  The library uploads pass k + 1 and downloads pass k - 1 on a copy stream
    under pass k's kernels (csrc/reid_internal.h host_passes); sources: one stacked uint8 array in pinned memory (reid_host_alloc),
    the same array in pageable memory, and a Python list of per-crop views of the pinned array (the reference's argument type)."""
    from reid_amd import synth
    from reid_amd.extractor import Extractor
    res = {}
    try:
        eng = job.eng
        eng.set_chunk(args.chunk)
        n = args.crops
        ext = Extractor(synth.seres18_state_dict(0, gem_p=3.0))
        pageable = synth.crops_u8(n, seed=1)
        pinned = eng.pinned(pageable.nbytes).reshape(pageable.shape)
        pinned[...] = pageable
        value = float(out.get("value") or 0.0)

        def rate(arg, count, reps):
            ext(arg)                                           # warm-up: workspaces, the copy stream, its events
            t0 = time.perf_counter()
            for _ in range(reps):
                feats = ext(arg)
            el = (time.perf_counter() - t0) / reps
            assert feats.shape == (count, 512) and np.isfinite(feats).all()
            return {"crops": count, "ms_per_call": round(el * 1e3, 3), "crops_per_s": round(count / el, 1),
                    "fraction_of_value": round(count / el / value, 4) if value else None}
        res["precision"] = ext.precision
        res["pass_size"] = args.chunk
        res["pinned"] = rate(pinned, n, 5)
        res["crops_per_s"] = res["pinned"]["crops_per_s"]
        res["fraction_of_value"] = res["pinned"]["fraction_of_value"]
        res["pinned_256"] = rate(pinned[:256], min(256, n), 20)
        res["pageable"] = rate(pageable, n, 3)
        res["pageable_256"] = rate(pageable[:256], min(256, n), 20)
        views = [pinned[i] for i in range(n)]
        res["list_of_views_pinned"] = rate(views, n, 3)         # + the per-crop Python checks of the list argument
        res["h2d_bytes_per_call"] = int(pageable.nbytes)
        res["note"] = ("Extractor.__call__ end to end on host memory; transfers overlap the kernels pass by pass (pass k+1 up, pass k-1 "
                       "down under pass k); the first pass's upload and the last pass's download are exposed")
    except Exception as e:     # noqa: BLE001
        res["error"] = "%s: %s" % (type(e).__name__, e)
    return res


_RESULT_FD = None


def emit(line):
    """The ONE line of the contract goes to the process's original stdout; everything else any library prints to fd 1 (RCCL's
    version banner at NCCL_DEBUG=WARN, ROCm notices) was redirected to stderr in main()."""
    data = (line + "\n").encode()
    if _RESULT_FD is None:
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
    else:
        os.write(_RESULT_FD, data)


def self_launch(argv, gpus):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start the N ranks as a CHILD process
    (python -m torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1), pass its stdout (the one JSON line of rank 0)
    and stderr through, and return its exit code.  Runs before this process has touched torch, HIP or the library - nothing is
    exec'ed or restarted in place.  The reference's own multi-GPU entry points are single commands too (reid/faiss_utils.py:121-135
    IndexShards, image_reid_inference.py:211 DataParallel)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_cores() // gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print("[bench] --gpus %d without a launcher environment: starting %s" % (gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def has_error(obj):
    return isinstance(obj, dict) and ("error" in obj or any(has_error(v) for v in obj.values()))


def main(argv=None):
    global _RESULT_FD
    argv = sys.argv[1:] if argv is None else argv
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything, not only the headline: the other arithmetic modes, roofline and per-kernel "
                         "figures, parity of the modes, cpu_baseline, and with --workload all the other configurations")
    ap.add_argument("--workload", choices=["all", "embed", "batch256", "swin", "tracking", "market", "host"], default="all",
                    help="all (default) = BASELINE configs[1] as the headline + (--full) the other configurations as sub-objects of "
                         "the same line; embed = configs[1] alone; with --full only: batch256 / swin / tracking / market = that "
                         "configuration as its own line; host = configs[1] in the headline arithmetic only + the host_path "
                         "sub-object (Extractor on host crops)")
    ap.add_argument("--crops", type=int, default=4096, help="crops (images) per GPU per step (BASELINE config 2 / 3: 4096)")
    ap.add_argument("--frames", type=int, default=600, help="--workload tracking: frames of the stream")
    ap.add_argument("--match-stream", type=int, default=1,
                    help="tracking: 0 = cost / update stages of the frame pipeline on the compute stream (rounds 3-5) instead of a stream of their own; 2 = on their own stream even beside a communicator")
    ap.add_argument("--chunk", type=int, default=int(os.environ.get("REID_CHUNK", "1024")))
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline legs")
    ap.add_argument("--cameras", type=int, default=2, help="--workload tracking, one GPU: also run this many concurrent camera streams")
    ap.add_argument("--no-pipeline", action="store_true", help="--workload tracking: one synchronous call per operation (A/B)")
    ap.add_argument("--single", action="store_true", help="--full: measure only --precision (skip the other arithmetic)")
    ap.add_argument("--precision", choices=["f32", "f16", "f16x3"], default=os.environ.get("REID_PRECISION", "f16x3"),
                    help="arithmetic of the headline: f16x3 (default) = fp32-class - fp32 storage, every convolution as "
                         "three f16 matrix-core products per multiply on hi/lo-split operands with fp32 accumulation; it meets the "
                         "exact-fp32 mode's parity bar (stage taps < 2e-5 of the reference, 1 - cos < 1e-5, no arg-min differs where the "
                         "reference's top-2 gap exceeds 2e-6 and none at all on the realistic config-1 set: tests/test_gpu_parity.py); f32 = exact fp32 MFMA (side run f32_path); f16 = fp16 storage / "
                         "fp32 accumulate (side run f16_path, north_star's 1e-3 cosine tolerance)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (fp32 / fp64, "
                         "at most 64 MB in all: a larger output as a fixed sample of its rows); default line: the headline's "
                         "embeddings and distance matrix.  Not for --workload tracking")
    args = ap.parse_args(argv)
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if not args.full and args.workload not in ("all", "embed"):
        ap.error("--workload %s: only with --full" % args.workload)
    if args.dump_outputs and args.workload == "tracking":
        ap.error("--dump-outputs: not available for --workload tracking")
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(argv, args.gpus)
    if args.workload == "batch256":
        args.crops = 256

    # dmabuf IPC for RCCL between the ranks of a node (the pool's driver has no legacy IPC: hipIpcGetMemHandle fails without it);
    # must be in the environment before the first HIP call
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.stdout.flush()
    _RESULT_FD = os.dup(1)
    os.dup2(2, 1)                      # native libraries that write to fd 1 now write to stderr

    job = Job(args)
    rc = 0
    try:
        def run_host(job_, a):
            a.single, a.no_cpu = True, True
            o = run_embed(job_, a)
            if o is not None and job_.world == 1:
                o["host_path"] = host_path(job_, o, a)
            return o
        fn = {"all": run_all if args.full else run_embed, "embed": run_embed, "batch256": run_embed, "swin": run_swin, "tracking": run_tracking,
              "market": run_market, "host": run_host}[args.workload]
        out = fn(job, args)
        if out is not None:
            emit(json.dumps(out))
            if has_error(out):         # a sub-workload that raised is in the line as {"error": ...}: the run did not succeed
                rc = 4
        job.barrier()
    finally:
        job.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
