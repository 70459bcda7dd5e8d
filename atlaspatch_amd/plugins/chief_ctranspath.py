"""``--feature-plugin`` module: the reference's ``chief-ctranspath`` (a Swin-Tiny with a convolutional stem,
models/patch/chief_ctranspath.py) on the native HIP kernels.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors chief-ctranspath \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.chief_ctranspath as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/chief-ctranspath.{safetensors,pt,pth} (the CHIEF_CTransPath checkpoint as it is, timm keys or
transformers SwinModel keys for the stages), or ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.
"""
from atlaspatch_amd.encoders.swin import register_chief_ctranspath


def register_feature_extractors(registry, device, dtype, num_workers):
    register_chief_ctranspath(registry, device=device, dtype=dtype, num_workers=num_workers)
