"""The ResNet18-IBN family in the three arithmetic modes: crops/s of one pass of 1024 crops (the bench's pass size) for seres18_ibn,
cares18_ibn and emares18_ibn in exact fp32 (mode 0), fp16 storage (mode 1) and fp32-class (mode 2), all in one call.
    python tools/bench_siblings.py      -> one JSON line (profiles/siblings_f16_bench.json)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine

n = 1024
eng = get_engine(0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
eng.set_stream(stream.cuda_stream)
eng.set_chunk(n)
x = torch.from_numpy(synth.smooth_crops_u8(64, 1)).cuda().repeat(n // 64, 1, 1, 1).contiguous()
emb = torch.empty((n, 512), dtype=torch.float32, device="cuda")
out = {"workload": "ResNet18-IBN family, %d crops 256x128 in one pass, crops/s" % n}
for name, sd_fn in (("seres18_ibn", synth.seres18_state_dict), ("cares18_ibn", synth.cares18_state_dict), ("emares18_ibn", synth.emares18_state_dict)):
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(sd_fn(0))[:2])
    for label, mode in (("f32", 0), ("f16", 1), ("f16x3", 2)):
        eng.set_precision(mode)
        for _ in range(2):
            eng.embed_u8_dev(x.data_ptr(), n, emb.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng.embed_u8_dev(x.data_ptr(), n, emb.data_ptr())
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / 3
        eng.profile_reset()
        eng.profile(True)
        eng.embed_u8_dev(x.data_ptr(), n, emb.data_ptr())
        torch.cuda.synchronize()
        gm, ew = eng.profile_get(_ffi.K_CONV_GEMM), eng.profile_get(_ffi.K_ELEMENTWISE)
        eng.profile(False)
        out["%s_%s" % (name, label)] = {"crops_per_s": round(n / el, 1), "ms": round(el * 1e3, 2), "gemm_ms": round(gm["ms"], 2),
                                        "other_ms": round(ew["ms"], 2), "other_launches": ew["launches"]}
    eng.set_precision(0)
for name in ("cares18_ibn", "emares18_ibn"):
    out["%s_f16_over_f32" % name] = round(out[name + "_f16"]["crops_per_s"] / out[name + "_f32"]["crops_per_s"], 2)
print(json.dumps(out))
