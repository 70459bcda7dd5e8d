"""CPU restatement of the OpenAI CLIP "modified ResNet" image tower (the yardstick of the CLIP ResNet encoders), written from
the published architecture in plain torch.nn.functional on the canonical open_clip-key state dict, at any float dtype:

* stem: three 3x3 convolutions (the first of stride 2), each + BatchNorm (eval statistics, eps 1e-5) + ReLU, then a 2x2
  average pool;
* bottleneck blocks (expansion 4): conv1 1x1, conv2 3x3 of stride 1, a 2x2 average pool when the block's stride is 2, conv3 1x1;
  the shortcut is the identity or (average pool when the stride is 2) + 1x1 convolution + BatchNorm; ReLU(main + shortcut);
* attention-pool head: the mean token in front of the g x g map tokens, + positional embedding, the mean token as the only
  query over all tokens (heads of 64, scale 1 / 8), output projection.

``forward`` takes the unfolded checkpoint.  ``forward_folded`` takes the BatchNorm-folded parameters the engine is given
(``encoders.clip_resnet.fold_batchnorm``) and a ``store`` hook applied to every tensor the engine keeps in memory: with
``store = round to T`` and weights rounded to T it is the ideal-T pass that sets the 16-bit bounds of the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5
HEAD_DIM = 64


def _bn(x, sd, name):
    return F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"], sd[f"{name}.bias"],
                        False, 0.0, EPS)


def attention_pool(x, pos, wq, bq, wk, bk, wv, bv, wc, bc, store=lambda t: t):
    """x [n, C, g, g] -> [n, output_dim], every step written out (no fused attention call)."""
    n, c, h, w = x.shape
    tok = x.flatten(2).permute(0, 2, 1)                                  # [n, g g, C]
    tok = store(torch.cat([tok.mean(dim=1, keepdim=True), tok], dim=1) + pos[None])
    heads = c // HEAD_DIM
    q = store(tok[:, 0] @ wq.t() + bq).view(n, heads, HEAD_DIM)          # the mean token is the only query
    k = store(tok @ wk.t() + bk).view(n, -1, heads, HEAD_DIM)
    v = store(tok @ wv.t() + bv).view(n, -1, heads, HEAD_DIM)
    logits = torch.einsum("nhd,nthd->nht", q, k) * HEAD_DIM ** -0.5
    attn = torch.softmax(logits, dim=-1)
    out = store(torch.einsum("nht,nthd->nhd", attn, v).reshape(n, c))
    return store(out @ wc.t() + bc)


def forward(sd, x, *, depths):
    """x [n, 3, S, S] normalised, in the dtype of ``sd``.  Returns [n, output_dim]."""
    x = F.relu(_bn(F.conv2d(x, sd["conv1.weight"], stride=2, padding=1), sd, "bn1"))
    x = F.relu(_bn(F.conv2d(x, sd["conv2.weight"], padding=1), sd, "bn2"))
    x = F.relu(_bn(F.conv2d(x, sd["conv3.weight"], padding=1), sd, "bn3"))
    x = F.avg_pool2d(x, 2)
    for s, depth in enumerate(depths):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            stride = 2 if (s > 0 and b == 0) else 1
            y = F.relu(_bn(F.conv2d(x, sd[pre + "conv1.weight"]), sd, pre + "bn1"))
            y = F.relu(_bn(F.conv2d(y, sd[pre + "conv2.weight"], padding=1), sd, pre + "bn2"))
            if stride == 2:
                y = F.avg_pool2d(y, 2)
            y = _bn(F.conv2d(y, sd[pre + "conv3.weight"]), sd, pre + "bn3")
            if pre + "downsample.0.weight" in sd:
                sc = F.avg_pool2d(x, 2) if stride == 2 else x
                sc = _bn(F.conv2d(sc, sd[pre + "downsample.0.weight"]), sd, pre + "downsample.1")
            else:
                sc = x
            x = F.relu(y + sc)
    a = "attnpool."
    return attention_pool(x, sd[a + "positional_embedding"], sd[a + "q_proj.weight"], sd[a + "q_proj.bias"], sd[a + "k_proj.weight"],
                          sd[a + "k_proj.bias"], sd[a + "v_proj.weight"], sd[a + "v_proj.bias"], sd[a + "c_proj.weight"],
                          sd[a + "c_proj.bias"])


def trunk_folded(p, x, *, depths, store=lambda t: t, maps=None):
    """The convolutional part on folded parameters (``<conv>.weight`` / ``<conv>.bias``): x [n, Cin, S, S] -> the final map.
    ``maps`` (a list) receives every tensor the engine stores, in launch order."""
    def keep(t):
        t = store(t)
        if maps is not None:
            maps.append(t)
        return t

    def conv(t, name, stride=1, resid=None, relu=True):
        w = p[name + ".weight"]
        y = F.conv2d(t, w, p[name + ".bias"].to(t.dtype), stride=stride, padding=w.shape[-1] // 2)
        if resid is not None:
            y = y + resid
        return keep(F.relu(y) if relu else y)

    x = keep(x)
    x = conv(x, "conv1", stride=2)
    x = conv(x, "conv2")
    x = conv(x, "conv3")
    x = keep(F.avg_pool2d(x, 2))
    for s, depth in enumerate(depths):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            stride = 2 if (s > 0 and b == 0) else 1
            y = conv(x, pre + "conv1")
            y = conv(y, pre + "conv2")
            sc = x
            if stride == 2:
                sc = conv(keep(F.avg_pool2d(x, 2)), pre + "downsample", relu=False)
                y = keep(F.avg_pool2d(y, 2))
            elif pre + "downsample.weight" in p:
                sc = conv(x, pre + "downsample", relu=False)
            x = conv(y, pre + "conv3", resid=sc)
    return x


def forward_folded(p, x, *, depths, store=lambda t: t):
    """The whole network on folded parameters (``attnpool.pos``, ``attnpool.q|kv|c.weight|bias`` for the head)."""
    x = trunk_folded(p, x, depths=depths, store=store)
    c = x.shape[1]
    kvw, kvb = p["attnpool.kv.weight"].flatten(1), p["attnpool.kv.bias"].to(x.dtype)           # [2C, C, 1, 1] as the engine takes it
    return attention_pool(x, p["attnpool.pos"].to(x.dtype), p["attnpool.q.weight"].flatten(1), p["attnpool.q.bias"].to(x.dtype),
                          kvw[:c], kvb[:c], kvw[c:], kvb[c:], p["attnpool.c.weight"].flatten(1), p["attnpool.c.bias"].to(x.dtype),
                          store=store)


def preprocess(tile, *, size):
    """open_clip's transform for the ``openai`` tags on an HWC uint8 tile: Pillow BICUBIC resize of the shorter side to ``size``
    (skipped when it already is), centre crop, ToTensor, Normalize -> float32 [3, size, size]."""
    img = Image.fromarray(np.asarray(tile))
    w, h = img.size
    if min(w, h) != size:
        if w <= h:
            img = img.resize((size, int(size * h / w)), Image.BICUBIC)
        else:
            img = img.resize((int(size * w / h), size), Image.BICUBIC)
    w, h = img.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    arr = np.asarray(img)[top:top + size, left:left + size].astype(np.float32)
    x = torch.from_numpy(arr).permute(2, 0, 1) / 255.0
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def extract_batch(sd, tiles, *, depths, size):
    x = torch.stack([preprocess(t, size=size) for t in tiles])
    with torch.no_grad():
        return forward(sd, x, depths=depths).numpy()
