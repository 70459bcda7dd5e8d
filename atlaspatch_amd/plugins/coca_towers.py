"""``--feature-plugin`` module: the reference's ``omiclip`` (open_clip ``coca_ViT-L-14``, models/patch/omiclip.py) and
``conch_v15`` (CONCH v1.5 of the TITAN repository, models/patch/conch.py:67-112) on the native HIP kernels: ViT-L trunks whose
features come from open_clip's AttentionalPooler with eight 96-wide heads.  The reference only calls the two packages; both
architectures are restated from the public packages and are UNVERIFIED OFFLINE (``encoders/vit_archs.py::ARCHS``), and parity is
claimed against that restatement (tests/coca_reference.py), not against the packages.

    python -m atlaspatch_amd process SLIDE -o OUT --feature-extractors omiclip,conch_v15 --feature-precision float16 \
        --feature-plugin "$(python -c 'import atlaspatch_amd.plugins.coca_towers as m; print(m.__file__)')"

Weights: $ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth} -- omiclip: open_clip's state dict (``visual.*`` bare or prefixed, or
the whole CoCa model, whose text towers are dropped); conch_v15: ``trunk.*``, ``attn_pool_contrast.*``, ``ln_contrast.*``, bare
or under ``visual.`` / ``vision_encoder.`` -- or ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights.  omiclip also runs
with --feature-precision float32; conch_v15 (785 tokens) in float16 / bfloat16 only.
"""
from atlaspatch_amd.encoders.vit import register_coca_towers


def register_feature_extractors(registry, device, dtype, num_workers):
    register_coca_towers(registry, device=device, dtype=dtype, num_workers=num_workers)
