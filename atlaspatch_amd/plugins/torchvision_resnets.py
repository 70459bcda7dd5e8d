"""``--feature-plugin`` module: the reference's torchvision ResNet names (resnet18 / 34 / 50 / 101 / 152,
models/patch/resnet.py) on the native HIP convolution kernels.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors resnet50 \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.torchvision_resnets as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth} (torchvision or transformers ResNetModel keys), or
ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.
"""
from atlaspatch_amd.encoders.resnet import register_resnets


def register_feature_extractors(registry, device, dtype, num_workers):
    register_resnets(registry, device=device, dtype=dtype, num_workers=num_workers)
