"""``--feature-plugin`` module: the reference's ``medsiglip`` (transformers' SiglipVisionModel of google/medsiglip-448,
models/patch/medsiglip.py: a ViT without a class token, tanh GELU, attention-pooling head) on the native HIP kernels.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors medsiglip --feature-precision float16 \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.medsiglip as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/medsiglip.{safetensors,pt,pth} (the HF state dict: the vision tower alone, bare or with the
``vision_model.`` prefix, or the whole SiglipModel), or ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.  An optional
$ATLASPATCH_WEIGHTS_DIR/medsiglip.preprocessor_config.json (the processor config published with the checkpoint) overrides the
resize filter and the normalisation constants.  float16 / bfloat16 only.
"""
from atlaspatch_amd.encoders.vit import register_medsiglip


def register_feature_extractors(registry, device, dtype, num_workers):
    register_medsiglip(registry, device=device, dtype=dtype, num_workers=num_workers)
