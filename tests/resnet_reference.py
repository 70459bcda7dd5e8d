"""CPU restatement of the torchvision ResNet forward (the yardstick of the ResNet encoders): plain torch.nn.functional,
float32, BatchNorm unfolded (eval statistics, eps 1e-5), on the canonical torchvision-key state dict; the feature is the
flattened global average pool (the reference's fc = Identity, models/patch/resnet.py)."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-5


def _bn(x, sd, name):
    return F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"], sd[f"{name}.bias"],
                        False, 0.0, EPS)


def forward(sd, x, *, block, depths, stages_out=None):
    """x: float32 [n, 3, H, W] normalised.  Returns float32 [n, C]; ``stages_out`` (a list) receives the stem's and every
    stage's output."""
    x = F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)
    x = F.relu(_bn(x, sd, "bn1"))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    if stages_out is not None:
        stages_out.append(x)
    n_conv = 3 if block == "bottleneck" else 2
    for s, depth in enumerate(depths):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            stride = 2 if (s > 0 and b == 0) else 1
            y = x
            for i in range(1, n_conv + 1):
                w = sd[f"{pre}conv{i}.weight"]
                k = w.shape[-1]
                st = stride if (i == 2 if block == "bottleneck" else i == 1) else 1
                y = _bn(F.conv2d(y, w, stride=st, padding=k // 2), sd, f"{pre}bn{i}")
                if i < n_conv:
                    y = F.relu(y)
            if f"{pre}downsample.0.weight" in sd:
                sc = _bn(F.conv2d(x, sd[f"{pre}downsample.0.weight"], stride=stride), sd, f"{pre}downsample.1")
            else:
                sc = x
            x = F.relu(y + sc)
        if stages_out is not None:
            stages_out.append(x)
    return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)


def preprocess(tile, *, resize=256, crop=224):
    """torchvision ImageClassification(crop_size=224) on an HWC uint8 tile: Pillow BILINEAR resize of the shorter side to
    ``resize`` (skipped when it already is), centre crop, ToTensor, Normalize -> float32 [3, crop, crop]."""
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


def extract_batch(sd, tiles, *, block, depths):
    if len(tiles) == 0:
        return np.empty((0, 512 if block == "basic" else 2048), np.float32)
    x = torch.stack([preprocess(t) for t in tiles])
    with torch.no_grad():
        return forward(sd, x, block=block, depths=depths).numpy()
