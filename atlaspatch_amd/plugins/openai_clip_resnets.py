"""``--feature-plugin`` module: the reference's OpenAI CLIP ResNet names (clip_rn50 / clip_rn101 / clip_rn50x4 / clip_rn50x16 /
clip_rn50x64, models/patch/clip.py) on the native HIP kernels.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors clip_rn50 \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.openai_clip_resnets as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth} (open_clip / OpenAI CLIP keys: the visual tower, or the whole model
with its ``visual.`` prefix), or ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.
"""
from atlaspatch_amd.encoders.clip_resnet import register_clip_resnets


def register_feature_extractors(registry, device, dtype, num_workers):
    register_clip_resnets(registry, device=device, dtype=dtype, num_workers=num_workers)
