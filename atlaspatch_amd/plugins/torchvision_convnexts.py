"""``--feature-plugin`` module: the reference's torchvision ConvNeXt names (convnext_tiny / small / base / large,
models/patch/convnext.py) on the native HIP kernels.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors convnext_tiny \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.torchvision_convnexts as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth} (torchvision or transformers ConvNextModel keys), or
ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.
"""
from atlaspatch_amd.encoders.convnext import register_convnexts


def register_feature_extractors(registry, device, dtype, num_workers):
    register_convnexts(registry, device=device, dtype=dtype, num_workers=num_workers)
