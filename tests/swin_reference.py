"""Plain-torch restatement of the CHIEF-CTransPath forward (the yardstick of the Swin encoder): a Swin-Tiny with a
convolutional stem, written with torch.nn.functional on the canonical timm-key state dict (BatchNorm unfolded), sharing no code
with the product's adapter.  Runs in the dtype and on the device of its input (float32 on the CPU as the yardstick; float16 /
bfloat16 on the GPU as the reference runs those precisions).

Stem: conv 3x3 s2 p1 (no bias) + BatchNorm (eps 1e-5, running statistics, folded into the convolution in float32) + ReLU,
twice (3 -> E/8 -> E/4), conv 1x1 (E/4 -> E, bias), LayerNorm.  Four stages; stages 2-4 open with patch merging
(x[0::2,0::2] | x[1::2,0::2] | x[0::2,1::2] | x[1::2,1::2], LayerNorm(4C), Linear(4C -> 2C, no bias)).  Block j: shift 0 (j
even, or the map is one window) or 3; x += proj(WA(LN1(x))); x += fc2(GELU_erf(fc1(LN2(x)))).  Final LayerNorm, mean over the
tokens.  Every LayerNorm has eps 1e-5."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-5
WS = 7
HEADS = (3, 6, 12, 24)
DEPTHS = (2, 2, 6, 2)


def fold_stem(sd):
    """[(weight, bias)] of the stem's two 3x3 convolutions with their BatchNorm folded in, float32."""
    out = []
    for conv, bn in ((0, 1), (3, 4)):
        w = sd[f"patch_embed.proj.{conv}.weight"].float()
        inv = sd[f"patch_embed.proj.{bn}.weight"].float() * torch.rsqrt(sd[f"patch_embed.proj.{bn}.running_var"].float() + EPS)
        out.append((w * inv[:, None, None, None],
                    sd[f"patch_embed.proj.{bn}.bias"].float() - sd[f"patch_embed.proj.{bn}.running_mean"].float() * inv))
    return out


def stem(sd, x):
    """x [n, 3, S, S] -> tokens [n, S/4, S/4, E] after patch_embed.norm."""
    p = lambda t: t.to(x.device, x.dtype)
    for w, b in fold_stem(sd):
        x = F.relu(F.conv2d(x, p(w), p(b), stride=2, padding=1))
    x = F.conv2d(x, p(sd["patch_embed.proj.6.weight"]), p(sd["patch_embed.proj.6.bias"]))
    x = x.permute(0, 2, 3, 1)
    return F.layer_norm(x, (x.shape[-1],), p(sd["patch_embed.norm.weight"]), p(sd["patch_embed.norm.bias"]), EPS)


def pair_bias(table):
    """relative_position_bias_table [169, heads] -> [heads, 49, 49], the way timm builds its index."""
    coords = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)     # [2, 49]
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (WS - 1)                              # [49, 49, 2]
    index = (rel[..., 0] * (2 * WS - 1) + rel[..., 1]).to(table.device)
    return table[index.view(-1)].view(WS * WS, WS * WS, -1).permute(2, 0, 1)


def region_mask(h, w, shift, device, dtype):
    """[windows, 49, 49]: -100 where two tokens of a window of the rolled map carry different region labels."""
    label = torch.zeros(h, w)
    count = 0
    for ys in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
        for xs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            label[ys, xs] = count
            count += 1
    win = label.view(h // WS, WS, w // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)
    diff = win[:, None, :] - win[:, :, None]
    return torch.where(diff != 0, torch.tensor(-100.0), torch.tensor(0.0)).to(device, dtype)


def window_attention(qkv, heads, shift, bias):
    """qkv [n, h, w, 3C] (q | k | v, head-major), bias [heads, 49, 49] -> [n, h, w, C]."""
    n, h, w, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    if shift:
        qkv = torch.roll(qkv, (-shift, -shift), (1, 2))
    win = qkv.view(n, h // WS, WS, w // WS, WS, 3, heads, d).permute(5, 0, 1, 3, 6, 2, 4, 7)
    win = win.reshape(3, n, (h // WS) * (w // WS), heads, WS * WS, d)
    q, k, v = win[0], win[1], win[2]
    attn = (q * d ** -0.5) @ k.transpose(-2, -1) + bias
    if shift:
        attn = attn + region_mask(h, w, shift, qkv.device, qkv.dtype)[None, :, None]
    out = F.softmax(attn, dim=-1) @ v                                            # [n, windows, heads, 49, d]
    out = out.view(n, h // WS, w // WS, heads, WS, WS, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, h, w, c)
    if shift:
        out = torch.roll(out, (shift, shift), (1, 2))
    return out


def stages(sd, x, *, depths=DEPTHS, heads=HEADS, branch_ratios=None):
    """tokens [n, H, W, E] (after patch_embed.norm) -> float [n, 8E]: the four stages, the final LayerNorm, the token mean.
    ``branch_ratios`` (a list) receives, per block, ||branch|| / ||residual input|| of the attention and the MLP half."""
    p = lambda key: sd[key].to(x.device, x.dtype)
    ln = lambda t, pre: F.layer_norm(t, (t.shape[-1],), p(pre + ".weight"), p(pre + ".bias"), EPS)
    for s, depth in enumerate(depths):
        if s > 0:
            d = f"layers.{s}.downsample."
            x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
            x = F.linear(ln(x, d + "norm"), p(d + "reduction.weight"))
        for j in range(depth):
            b = f"layers.{s}.blocks.{j}."
            shift = WS // 2 if (j % 2 == 1 and min(x.shape[1:3]) > WS) else 0
            qkv = F.linear(ln(x, b + "norm1"), p(b + "attn.qkv.weight"), p(b + "attn.qkv.bias"))
            a = window_attention(qkv, heads[s], shift, pair_bias(p(b + "attn.relative_position_bias_table")))
            a = F.linear(a, p(b + "attn.proj.weight"), p(b + "attn.proj.bias"))
            if branch_ratios is not None:
                branch_ratios.append(float(a.norm() / x.norm()))
            x = x + a
            m = F.gelu(F.linear(ln(x, b + "norm2"), p(b + "mlp.fc1.weight"), p(b + "mlp.fc1.bias")))
            m = F.linear(m, p(b + "mlp.fc2.weight"), p(b + "mlp.fc2.bias"))
            if branch_ratios is not None:
                branch_ratios.append(float(m.norm() / x.norm()))
            x = x + m
    return ln(x, "norm").flatten(1, 2).mean(1)


def forward(sd, x, *, depths=DEPTHS, heads=HEADS, branch_ratios=None):
    """x: [n, 3, S, S] normalised (any float dtype / device).  Returns [n, 8E] in x's dtype."""
    return stages(sd, stem(sd, x), depths=depths, heads=heads, branch_ratios=branch_ratios)


def preprocess(tile):
    """transforms.Resize(224) on an HWC uint8 tile (Pillow BILINEAR resize of the shorter side to 224, skipped when it already
    is; no crop), ToTensor, Normalize -> float32 [3, H, W]."""
    img = Image.fromarray(np.asarray(tile))
    w, h = img.size
    if min(w, h) != 224:
        if w <= h:
            img = img.resize((224, int(224 * h / w)), Image.BILINEAR)
        else:
            img = img.resize((int(224 * w / h), 224), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(img).astype(np.float32)).permute(2, 0, 1) / 255.0
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def extract_batch(sd, tiles, *, depths=DEPTHS, heads=HEADS, device="cpu", dtype=torch.float32):
    """float32 numpy [n, 8E]; ``device`` / ``dtype``: where and in which precision the network runs."""
    if len(tiles) == 0:
        return np.empty((0, sd["norm.weight"].shape[0]), np.float32)
    x = torch.stack([preprocess(t) for t in tiles]).to(device, dtype)
    with torch.no_grad():
        return forward(sd, x, depths=depths, heads=heads).float().cpu().numpy()
