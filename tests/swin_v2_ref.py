"""Test infrastructure: CPU restatement of the reference's Swin-T ``version="v2"`` eval-mode forward as plain functional torch ops on a
``state_dict`` - what oracle/swin.py is for v1, in our own wording (no einops, no timm, no ``nn.Module`` of the reference).  Pinned
against the reference's own class by tests/golden/swin_v2.npz (tools/gen_golden_swin_v2.py) in tests/test_swin_v2_host.py; the GPU
tests then use it for shapes the fixture does not hold, and ``window_attention`` / ``post_norm`` in float64 as the kernels' oracles.

Follows reid/backbones/swin_transformer.py: :165-189 log-spaced relative coordinates -> meta_mlp -> bias [heads][49][49]; :205-209
cosine attention, scale exp(min(logit_scale, ln 100)) per head; :85-92,238-246 post-norm blocks x + LN(f(x)).  The stem, patch
merging, top-down fusion and tail are v1's (oracle/swin.py).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.swin import HEAD_DIM, HEADS, LAYERS, WS, _lin, _t


def relative_coordinates_log(dtype=torch.float32):
    idx = torch.arange(WS * WS)
    coords = torch.stack([idx // WS, idx % WS], 0)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).reshape(-1, 2).to(dtype)
    return torch.sign(rel) * torch.log(1.0 + rel.abs())


def bias_table(sd, prefix, heads):
    """meta_mlp over the relative coordinates -> [heads][49][49] (query, key), in the dtype of the weights."""
    w1 = _t(sd, prefix + ".meta_mlp.fc1.weight")
    h = F.relu(F.linear(relative_coordinates_log(w1.dtype), w1, _t(sd, prefix + ".meta_mlp.fc1.bias")))
    out = F.linear(h, _t(sd, prefix + ".meta_mlp.fc2.weight"), _t(sd, prefix + ".meta_mlp.fc2.bias"))
    return out.transpose(1, 0).reshape(heads, WS * WS, WS * WS)


def scales(sd, prefix):
    return torch.clamp(_t(sd, prefix + ".logit_scale"), max=math.log(1.0 / 0.01)).exp()


def shift_masks(dtype):
    """create_mask (:95-108): -inf between the two sides of the seam of the last window row / column."""
    idx = torch.arange(WS * WS)
    neg = torch.tensor(float("-inf"), dtype=dtype)
    zero = torch.tensor(0.0, dtype=dtype)
    ul = torch.where(((idx // WS) >= WS - 3)[:, None] != ((idx // WS) >= WS - 3)[None, :], neg, zero)
    lr = torch.where(((idx % WS) >= WS - 3)[:, None] != ((idx % WS) >= WS - 3)[None, :], neg, zero)
    return ul, lr


def window_attention(qkv, heads, shifted, bias, scale):
    """qkv [b, H, W, 3 * heads * 32] of tokens in place (the cyclic shift happens here) -> [b, H, W, heads * 32], in qkv's dtype.
    bias [heads, 49, 49], scale [heads] (clamped and exponentiated)."""
    b, H, W, _ = qkv.shape
    C = heads * HEAD_DIM
    if shifted:
        qkv = torch.roll(qkv, shifts=(-3, -3), dims=(1, 2))
    nh, nw = H // WS, W // WS

    def split(t):
        t = t.reshape(b, nh, WS, nw, WS, heads, HEAD_DIM)
        return t.permute(0, 5, 1, 3, 2, 4, 6).reshape(b, heads, nh * nw, WS * WS, HEAD_DIM)

    q, k, v = (split(t) for t in qkv.chunk(3, dim=-1))
    dots = torch.matmul(F.normalize(q, dim=-1), F.normalize(k, dim=-1).transpose(-1, -2))
    dots = dots * scale.to(qkv.dtype).reshape(1, heads, 1, 1, 1)
    dots = dots + bias.to(qkv.dtype).reshape(1, heads, 1, WS * WS, WS * WS)
    if shifted:
        ul, lr = shift_masks(qkv.dtype)
        dots[:, :, -nw:] += ul
        dots[:, :, nw - 1::nw] += lr
    out = torch.matmul(dots.softmax(dim=-1), v)
    out = out.reshape(b, heads, nh, nw, WS, WS, HEAD_DIM).permute(0, 2, 4, 3, 5, 1, 6).reshape(b, H, W, C)
    if shifted:
        out = torch.roll(out, shifts=(3, 3), dims=(1, 2))
    return out


def post_norm(x, y, g, b):
    return x + F.layer_norm(y, (y.shape[-1],), g, b, 1e-5)


def _block(sd, prefix, x, heads, shifted):
    a, m = prefix + ".attention_block.fn", prefix + ".mlp_block.fn"
    qkv = _lin(sd, a + ".fn.to_qkv", x, bias=False)
    h = window_attention(qkv, heads, shifted, bias_table(sd, a + ".fn", heads), scales(sd, a + ".fn"))
    h = _lin(sd, a + ".fn.post_proj", _lin(sd, a + ".fn.to_out", h))
    x = post_norm(x, h, _t(sd, a + ".norm.weight"), _t(sd, a + ".norm.bias"))
    h = _lin(sd, m + ".fn.net.3", F.gelu(_lin(sd, m + ".fn.net.0", x)))
    return post_norm(x, h, _t(sd, m + ".norm.weight"), _t(sd, m + ".norm.bias"))


def forward(sd, img, taps=None, view_index=None, side_info_coeff=1.5):
    """img: float32 [N,3,H,W] torch tensor, H and W multiples of 224 -> (emb [N,96], logits [N,num_class]).  ``view_index`` (per image)
    adds side_info_coeff * side_info_embedding[view] to the stem output (swin_transformer.py:298-302), as in v1."""
    with torch.no_grad():
        x = F.conv2d(img, _t(sd, "sfe.conv1.weight"), _t(sd, "sfe.conv1.bias"), 2)
        a = F.instance_norm(x[:, :6].contiguous(), None, None, _t(sd, "sfe.norm.instancenorm.weight"),
                            _t(sd, "sfe.norm.instancenorm.bias"), True, 0.0, 1e-5)
        bb = F.batch_norm(x[:, 6:].contiguous(), _t(sd, "sfe.norm.batchnorm.running_mean"), _t(sd, "sfe.norm.batchnorm.running_var"),
                          _t(sd, "sfe.norm.batchnorm.weight"), _t(sd, "sfe.norm.batchnorm.bias"), False, 0.0, 1e-5)
        x = F.relu(F.conv2d(F.relu(torch.cat((a, bb), 1)), _t(sd, "sfe.conv2.weight"), _t(sd, "sfe.conv2.bias"), 2))
        sfe = _lin(sd, "sfe.fc", x.permute(0, 2, 3, 1))
        if view_index is not None:
            sfe = sfe + side_info_coeff * _t(sd, "sfe.side_info_embedding")[torch.as_tensor(np.asarray(view_index), dtype=torch.long)]
        if taps is not None:
            taps["sfe"] = sfe
        outs = []
        x = sfe
        for si in range(4):
            st = "stage%d" % (si + 1)
            if si > 0:
                n, h, w, c = x.shape
                u = x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c * 4)
                x = _lin(sd, st + ".patch_partition.linear", u)
            for li in range(LAYERS[si] // 2):
                x = _block(sd, "%s.layers.%d.0" % (st, li), x, HEADS[si], False)
                x = _block(sd, "%s.layers.%d.1" % (st, li), x, HEADS[si], True)
            outs.append(x)
            if taps is not None:
                taps[st] = x
        nchw = [o.permute(0, 3, 1, 2) for o in outs]
        f = nchw[3] + F.conv2d(sfe.permute(0, 3, 1, 2), _t(sd, "img_channel_align.weight"), _t(sd, "img_channel_align.bias"), 8)
        f = nchw[2] + F.conv_transpose2d(f, _t(sd, "stage4_channel_align.weight"), _t(sd, "stage4_channel_align.bias"), 2, 1)
        f = F.conv_transpose2d(f, _t(sd, "stage3_channel_align.weight"), _t(sd, "stage3_channel_align.bias"), 2, 1) + nchw[1]
        f = F.conv_transpose2d(f, _t(sd, "stage2_channel_align.weight"), _t(sd, "stage2_channel_align.bias"), 2, 1) + nchw[0]
        tok = F.layer_norm(f.flatten(2).permute(0, 2, 1), (96,), _t(sd, "norm.weight"), _t(sd, "norm.bias"), 1e-6)
        p = _t(sd, "avgpool.p")
        g = tok.clamp(min=1e-6).pow(p).mean(dim=1).pow(1.0 / p)
        if taps is not None:
            taps["norm"] = tok
            taps["gem"] = g
        emb = F.batch_norm(g, _t(sd, "bottleneck.running_mean"), _t(sd, "bottleneck.running_var"), _t(sd, "bottleneck.weight"),
                           _t(sd, "bottleneck.bias"), False, 0.0, 1e-5)
        logits = F.linear(emb, _t(sd, "mlp_head.0.weight"))
    return emb, logits


def embed(sd, imgs, bs=16):
    return torch.cat([forward(sd, torch.from_numpy(np.ascontiguousarray(imgs[i:i + bs])))[0] for i in range(0, len(imgs), bs)], 0).numpy()
