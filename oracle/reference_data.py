"""Stages the reference's trained weight files and its pre-processed sample inputs into oracle/_ref/  --  TEST INFRASTRUCTURE ONLY.

The reference ships `stereoDNN/models/<Model>/TensorRT/trt_weights{,_fp16}.bin` (written by scripts/tensorrt_model_builder.py:52-60,
read by sample_app/main.cpp:111-134) and `stereoDNN/sample_app/data/img_{left,right}.bin`.  They are megabytes each, too large for the
repository, so `__graft_entry__.build()` copies them next to the other reference-derived artefacts in oracle/_ref/ (git-ignored; it
travels with the built tree to where the GPU tests run).  redtail_amd/model_files.py looks them up there and raises when one is
missing: no test falls back to synthetic weights where it says the reference's.
"""
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")

# below stereoDNN/ in the reference -> below oracle/_ref/
FILES = [
    "models/ResNet-18_2D/TensorRT/trt_weights.bin",
    "models/ResNet-18_2D/TensorRT/trt_weights_fp16.bin",
    "models/NVTiny/TensorRT/trt_weights.bin",
    "models/NVTiny/TensorRT/trt_weights_fp16.bin",
    "models/NVSmall/TensorRT/trt_weights_fp16.bin",
    "sample_app/data/img_left.bin",
    "sample_app/data/img_right.bin",
]


def stage(reference=None):
    """Copies FILES from the reference tree into oracle/_ref/.  Returns the staged paths; a no-op (empty list) when the reference
    tree is absent or unreadable."""
    reference = reference or os.environ.get("RT_REFERENCE", "/root/reference")
    staged = []
    for rel in FILES:
        src, dst = os.path.join(reference, "stereoDNN", rel), os.path.join(REF_DIR, rel)
        if not os.path.exists(src):
            continue
        if not os.path.exists(dst) or os.path.getsize(dst) != os.path.getsize(src):
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(src, dst)
        staged.append(dst)
    return staged
