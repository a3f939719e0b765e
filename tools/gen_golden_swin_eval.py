"""Generates tests/golden/swin_eval.npz from the REFERENCE's own swin_t, v1 and v2 (CPU only; run where the reference tree is).

    python tools/gen_golden_swin_eval.py --reference /path/to/reference

The evaluation script's Swin path (reid/image_reid_inference.py --backbone swin_v1 | swin_v2 [--sie], :145-152, :202-208) cannot be
imported as a whole (onnxruntime, cv2, datasets), so its glue is restated here line by line, as oracle/gen_golden.py gen_e2e does for
the ResNet: model(cat(img, flip(img)) [, cam.repeat(2)]) -> cat(normalize(first output), normalize(second output)) per view (:112-123)
-> normalize((plain + mirrored) / 2) (:252-253).  The Swin returns (logits, x_norm) in eval mode (swin_transformer.py:422-423), so a
row is [normalize(logits) (751) | normalize(x_norm) (96)].  timm / torchvision stand-ins as in tools/gen_golden_swin_v2.py; nothing of
the reference is written to the repository: the fixture holds numbers its classes produced.

Weights: synth.swin_state_dict(0, views=6, version=...) loaded strict=True into swin_t(camera=6, sequence=0, side_info=True).
Keys carry the suffix _v1 / _v2.

(a) descriptors, fp32, and the same from model.double() (suffix _f64 before the version):
      a4_*   4 images synth.images_f32(4, 5, h=448, w=224) with view_index [0, 3, 5, 1]
      a3_*   3 images synth.images_f32(3, 6) (224 x 224) without side information
      *_tta / *_plain / *_mirror   the TTA descriptor, the plain view's and the mirrored view's rows
      *_xn1 / *_xn2 / *_lg1 / *_lg2   x_norm and logits of the plain / mirrored view
(b) effect sizes of the 4-image set (what the tests' bars are conditions on):
      ref_noise     max |fp32 - float64| of the TTA descriptor
      tta_effect    max |TTA descriptor - normalize(plain-view descriptor)|
      side_effect   max |TTA descriptor with view_index - without|
    The generator asserts ref_noise * 100 < min(tta_effect, side_effect) / 16, the bar of the GPU test against these descriptors.
(c) the chain: labels of synth.e2e_problem(seed, n_ids=6, n_cams=4, n_gallery=48, n_query=12), images identity_images_f32(labels, cams,
    seed + 1 / seed + 2, h=448, w=224), use_side on (the cameras are the view indices), the links and taps of gen_e2e (key prefix
    chain_; rows every chain_row_step-th).  chain_noise_<link>: the reference's own fp32-vs-float64 deviation per link - the model and
    diminish_camera_bias / smooth_tracklets run in float64; compute_jaccard_distance holds float32 matrices inside, so its entry is the
    deviation of its result on the float64 chain's features from the fp32 chain's.  A seed is taken only if every link's noise is under a
    quarter of the GPU test's bar for it (desc 2e-5, debiased 5e-5, jaccard 2e-4, smoothed 5e-5) and chain_eps_margin is at least five
    Jaccard bars, for both versions; otherwise the next of CHAIN_SEEDS is tried and the choice is printed.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "swin_eval.npz")
VIEWS = 6
VIEW_INDEX = (0, 3, 5, 1)
CHAIN_SEEDS = (100, 101, 102, 103, 104, 105)
CHAIN_SIZES = dict(n_ids=6, n_cams=4, n_gallery=48, n_query=12)
CHAIN_ROW_STEP = 3
BARS = {"desc": 2e-5, "debiased": 5e-5, "jaccard": 2e-4, "smoothed": 5e-5}


def descriptors(model, x, view_index=None):
    """inference_efficient (:112-123) for one batch: (plain rows, mirrored rows, first output, second output), the model's dtype."""
    with torch.no_grad():
        img = torch.cat((x, torch.flip(x, dims=[3])), dim=0)
        if view_index is None:
            embeddings, outputs = model(img)
        else:
            embeddings, outputs = model(img, view_index.repeat(2))
        rows = torch.cat((F.normalize(embeddings, dim=1), F.normalize(outputs, dim=1)), dim=1)
    h = len(rows) >> 1
    return rows[:h], rows[h:], embeddings, outputs


def part_a(model, tag, x_np, view_index, ver, out):
    x = torch.from_numpy(x_np)
    vi = None if view_index is None else torch.tensor(view_index, dtype=torch.long)
    res = {}
    for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
        d1, d2, logits, x_norm = descriptors(model.to(dtype), x.to(dtype), vi)
        n = len(d1)
        res[suffix] = {"tta": F.normalize((d1 + d2) / 2.0, dim=1), "plain": d1, "mirror": d2, "xn1": x_norm[:n], "xn2": x_norm[n:], "lg1": logits[:n],
                       "lg2": logits[n:]}
        for k, v in res[suffix].items():
            if suffix == "" or k in ("tta", "plain", "mirror"):
                out["%s_%s%s_%s" % (tag, k, suffix, ver)] = v.numpy()
    model.float()
    return res


def chain(model, prob, g_img, q_img, dtype, eps=None, pseudo=None):
    """image_reid_inference.py:238-322 with use_side, in `dtype`; returns the taps (full size) and cmc / mAP."""
    from sklearn.cluster import DBSCAN
    from reid.inference_utils import diminish_camera_bias, smooth_tracklets
    from reid.faiss_utils import compute_jaccard_distance
    from reid.evaluate import evaluate_all
    model = model.double() if dtype == torch.float64 else model.float()

    def inference_efficient(images, cams):
        t1, t2 = [], []
        for i in range(0, len(images), 16):
            d1, d2, _, _ = descriptors(model, torch.from_numpy(images[i:i + 16]).to(dtype), torch.from_numpy(cams[i:i + 16]))
            t1.append(d1)
            t2.append(d2)
        return torch.cat(t1, dim=0), torch.cat(t2, dim=0)

    def ev(q, g):
        with contextlib.redirect_stdout(io.StringIO()):
            cmc, ap = evaluate_all(q.float(), torch.from_numpy(prob["ql"]), torch.from_numpy(prob["qc"]), g.float(), torch.from_numpy(prob["gl"]),
                                   torch.from_numpy(prob["gc"]))
        return cmc.numpy().astype(np.float32), np.float64(ap)

    g1, g2 = inference_efficient(g_img, prob["gc"])
    gallery = F.normalize((g1 + g2) / 2.0, dim=1)
    q1, q2 = inference_efficient(q_img, prob["qc"])
    query = F.normalize((q1 + q2) / 2.0, dim=1)
    ng = gallery.shape[0]
    merged = torch.cat((gallery, query), dim=0)
    merged_cams = torch.cat((torch.from_numpy(prob["gc"]), torch.from_numpy(prob["qc"])), dim=0)
    merged_seqs = torch.cat((torch.from_numpy(prob["gs"]), torch.from_numpy(prob["qs"])), dim=0)
    t = {"desc": merged.numpy().copy()}
    merged = diminish_camera_bias(merged, merged_cams)
    t["debiased"] = merged.numpy().copy()
    dists = compute_jaccard_distance(merged.float(), print_flag=False, search_option=3)
    dists[dists < 0] = 0.
    t["jaccard"] = dists.astype(np.float32).copy()
    if eps is None:      # gen_e2e's rule: the middle of the widest gap between neighbouring distances inside [0.45, 0.55]
        vals = np.unique(dists[(dists > 0.45) & (dists < 0.55)].astype(np.float64))
        gap = int(np.argmax(np.diff(vals)))
        eps = float((vals[gap] + vals[gap + 1]) / 2)
    t["eps"] = eps
    t["eps_margin"] = float(np.abs(dists - eps).min())
    if pseudo is None:
        pseudo = DBSCAN(eps=eps, min_samples=min(10, CHAIN_SIZES["n_cams"] + 1), metric="precomputed", n_jobs=-1).fit_predict(dists)
    t["pseudo_labels"] = np.asarray(pseudo).astype(np.int32)
    num_labels = max(pseudo) + 1
    merged_seqs = merged_seqs * num_labels + torch.from_numpy(np.asarray(pseudo).astype(np.int64))
    merged = smooth_tracklets(merged, merged_seqs, torch.from_numpy(np.asarray(pseudo) != -1))
    t["smoothed"] = merged.numpy().copy()
    t["cmc"], t["map"] = ev(merged[ng:], merged[:ng])
    model.float()
    return t


def chain_problem(seed):
    from reid_amd import synth
    prob = synth.e2e_problem(seed, **CHAIN_SIZES)
    g_img = synth.identity_images_f32(prob["gl"], prob["gc"], seed + 1, h=448, w=224)
    q_img = synth.identity_images_f32(prob["ql"], prob["qc"], seed + 2, h=448, w=224)
    return prob, g_img, q_img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds reid/backbones/swin_transformer.py)")
    args = ap.parse_args()
    from reid_amd import synth
    import gen_golden_swin_v2 as v2gen
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden
    v2gen._stand_ins(args.reference)
    gen_golden._faiss_stub()
    from reid.backbones.swin_transformer import swin_t

    torch.manual_seed(0)
    models = {}
    for ver in ("v1", "v2"):
        sd_np = synth.swin_state_dict(0, views=VIEWS, version=ver)
        model = swin_t(num_classes=751, loss="triplet", camera=VIEWS, sequence=0, side_info=True, version=ver)
        assert list(model.state_dict()) == list(sd_np)
        res = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        models[ver] = model.eval()

    out = {"view_index": np.array(VIEW_INDEX, np.int32), "views": np.int64(VIEWS)}
    for ver, model in models.items():
        a4 = part_a(model, "a4", synth.images_f32(4, 5, h=448, w=224), VIEW_INDEX, ver, out)
        part_a(model, "a3", synth.images_f32(3, 6), None, ver, out)
        noside = part_a(model, "a4ns", synth.images_f32(4, 5, h=448, w=224), None, ver, {})
        tta64 = a4["_f64"]["tta"]
        ref_noise = float((a4[""]["tta"].double() - tta64).abs().max())
        tta_effect = float((tta64 - F.normalize(a4["_f64"]["plain"], dim=1)).abs().max())
        side_effect = float((tta64 - noside["_f64"]["tta"]).abs().max())
        views_apart = float((a4["_f64"]["plain"] - a4["_f64"]["mirror"]).abs().max())
        print("%s: ref_noise %.2e  tta_effect %.2e  side_effect %.2e  plain vs mirrored %.2e  max |d| %.3f" %
              (ver, ref_noise, tta_effect, side_effect, views_apart, float(tta64.abs().max())))
        assert ref_noise * 100 < min(tta_effect, side_effect) / 16, "the reference's own noise is not far inside the bar"
        out.update({"ref_noise_" + ver: np.float64(ref_noise), "tta_effect_" + ver: np.float64(tta_effect),
                    "side_effect_" + ver: np.float64(side_effect)})

    for seed in CHAIN_SEEDS:
        prob, g_img, q_img = chain_problem(seed)
        if len(np.unique(np.concatenate([prob["gc"], prob["qc"]]))) < CHAIN_SIZES["n_cams"]:
            print("chain seed %d: a camera without rows" % seed)
            continue
        good, found = True, {}
        for ver, model in models.items():
            t32 = chain(model, prob, g_img, q_img, torch.float32)
            t64 = chain(model, prob, g_img, q_img, torch.float64, eps=t32["eps"], pseudo=t32["pseudo_labels"])
            noise = {k: float(np.abs(t32[k].astype(np.float64) - t64[k]).max()) for k in BARS}
            ok = all(noise[k] <= BARS[k] / 4 for k in BARS) and t32["eps_margin"] >= 5 * BARS["jaccard"]
            print("chain seed %d %s: noise %s | eps %.6f margin %.2e | %d clusters, %d noise points | Rank-1 %.4f mAP %.4f -> %s" %
                  (seed, ver, {k: "%.1e" % v for k, v in noise.items()}, t32["eps"], t32["eps_margin"], int(t32["pseudo_labels"].max()) + 1,
                   int((t32["pseudo_labels"] == -1).sum()), t32["cmc"][0], t32["map"], "ok" if ok else "rejected"))
            found[ver] = (t32, noise)
            good = good and ok
            if not good:
                break
        if good:
            break
    else:
        raise SystemExit("no chain seed keeps the reference inside a quarter of every bar")
    print("chain seed taken:", seed)
    out.update({"chain_seed": np.int64(seed), "chain_row_step": np.int64(CHAIN_ROW_STEP)})
    for k, v in CHAIN_SIZES.items():
        out["chain_" + k] = np.int64(v)
    for ver, (t, noise) in found.items():
        for k in ("desc", "debiased", "jaccard", "smoothed"):
            out["chain_%s_%s" % (k, ver)] = t[k][::CHAIN_ROW_STEP].astype(np.float32).copy()
            out["chain_noise_%s_%s" % (k, ver)] = np.float64(noise[k])
        out["chain_eps_" + ver], out["chain_eps_margin_" + ver] = np.float64(t["eps"]), np.float64(t["eps_margin"])
        out["chain_pseudo_labels_" + ver] = t["pseudo_labels"]
        out["chain_cmc_" + ver], out["chain_map_" + ver] = t["cmc"], t["map"]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
