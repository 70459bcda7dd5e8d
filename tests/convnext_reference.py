"""CPU restatement of the torchvision ConvNeXt forward (the yardstick of the ConvNeXt encoders): plain torch.nn.functional,
float32, on the canonical torchvision-key state dict (layer_scale unfolded); the feature is the flattened global average pool
of the last stage, WITHOUT the head's LayerNorm (the reference replaces the whole classifier, models/patch/convnext.py).
Every LayerNorm has eps 1e-6 and the GELU is the erf form; stochastic depth is the identity in eval."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-6


def _ln_channels(x, w, b):
    """LayerNorm over the channels of an NCHW tensor (torchvision's LayerNorm2d)."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, EPS).permute(0, 3, 1, 2)


def forward(sd, x, *, depths, branch_ratios=None):
    """x: float32 [n, 3, H, W] normalised.  Returns float32 [n, C_last].  ``branch_ratios`` (a list) receives, per block,
    ||branch|| / ||residual input|| over the batch."""
    x = F.conv2d(x, sd["features.0.0.weight"], sd["features.0.0.bias"], stride=4)
    x = _ln_channels(x, sd["features.0.1.weight"], sd["features.0.1.bias"])
    for s, depth in enumerate(depths):
        if s > 0:
            d = f"features.{2 * s}."
            x = _ln_channels(x, sd[d + "0.weight"], sd[d + "0.bias"])
            x = F.conv2d(x, sd[d + "1.weight"], sd[d + "1.bias"], stride=2)
        for j in range(depth):
            p = f"features.{2 * s + 1}.{j}."
            c = x.shape[1]
            y = F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], padding=3, groups=c)
            y = y.permute(0, 2, 3, 1)
            y = F.layer_norm(y, (c,), sd[p + "block.2.weight"], sd[p + "block.2.bias"], EPS)
            y = F.gelu(F.linear(y, sd[p + "block.3.weight"], sd[p + "block.3.bias"]))
            y = F.linear(y, sd[p + "block.5.weight"], sd[p + "block.5.bias"])
            y = y.permute(0, 3, 1, 2) * sd[p + "layer_scale"]
            if branch_ratios is not None:
                branch_ratios.append(float(y.norm() / x.norm()))
            x = x + y
    return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)


def preprocess(tile, *, resize, crop=224):
    """torchvision ImageClassification(crop_size=224, resize_size=resize) on an HWC uint8 tile: Pillow BILINEAR resize of
    the shorter side to ``resize`` (skipped when it already is), centre crop, ToTensor, Normalize -> float32 [3, crop, crop]."""
    img = Image.fromarray(np.asarray(tile))
    w, h = img.size
    if min(w, h) != resize:
        if w <= h:
            img = img.resize((resize, int(resize * h / w)), Image.BILINEAR)
        else:
            img = img.resize((int(resize * w / h), resize), Image.BILINEAR)
    w, h = img.size
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    arr = np.asarray(img)[top:top + crop, left:left + crop].astype(np.float32)
    x = torch.from_numpy(arr).permute(2, 0, 1) / 255.0
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def extract_batch(sd, tiles, *, depths, resize):
    if len(tiles) == 0:
        return np.empty((0, sd["features.0.0.weight"].shape[0] * 8), np.float32)
    x = torch.stack([preprocess(t, resize=resize) for t in tiles])
    with torch.no_grad():
        return forward(sd, x, depths=depths).numpy()
