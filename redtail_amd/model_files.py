"""Where the reference's trained weight files and sample data are found inside this repository.

The reference ships `stereoDNN/models/<Model>/TensorRT/trt_weights{,_fp16}.bin` (written by
scripts/tensorrt_model_builder.py:52-60, read by sample_app/main.cpp:111-134).  They are too large for the repository:
`__graft_entry__.build()` stages them from the reference tree into `oracle/_ref/models/` (oracle/reference_data.py;
git-ignored like every other reference-derived artefact, and it travels with the built tree), and tests look them up
through `weight_file()`, which raises when a file is missing: there is no silent fall-back to synthetic weights
anywhere a test says "real weights".  The sample application's stereo pair and the reference's plugin-test tensors are
stored in the repository itself (tests/golden/).
"""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")               # staged by build() where the reference tree exists
WEIGHT_DIR = os.path.join(ROOT, "weights", "_ref")           # git-ignored: files unpacked from tests/golden/

# (model id of include/rt_stereo_net.h, fp16 file?) -> path below stereoDNN/models
FILES = {
    ("resnet18_2D", False): "ResNet-18_2D/TensorRT/trt_weights.bin",
    ("resnet18_2D", True): "ResNet-18_2D/TensorRT/trt_weights_fp16.bin",
    ("nvtiny", False): "NVTiny/TensorRT/trt_weights.bin",
    ("nvtiny", True): "NVTiny/TensorRT/trt_weights_fp16.bin",
    ("nvsmall", True): "NVSmall/TensorRT/trt_weights_fp16.bin",     # the reference ships no fp32 file
}


def _write_atomic(path, data):
    """writes `data` to `path` through a temporary file, so that concurrent callers (test ranks) never see a partial file"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = "%s.%d.tmp" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def sample_image(side):
    """the reference sample application's left / right PNG (sample_app/data/img_<side>.png)"""
    path = os.path.join(GOLDEN_DIR, "sample", "img_%s.png" % side)
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing" % path)
    return path


def sample_bin(side):
    """the reference's own pre-processed network input for that image (sample_app/data/img_<side>.bin: 3 x 321 x 1025 float32), or None"""
    path = os.path.join(REF_DIR, "sample_app", "data", "img_%s.bin" % side)
    return path if os.path.exists(path) else None


def tests_data_dir():
    """stereoDNN/tests/data as the reference's plugin tests read it (int32 ndims, int32 dims[], float32 data[] per file,
    tests_main.cpp:259-275), unpacked from tests/golden/redtail_fixtures.npz into weights/_ref/tests_data/"""
    path = os.path.join(WEIGHT_DIR, "tests_data")
    with np.load(os.path.join(GOLDEN_DIR, "redtail_fixtures.npz")) as z:
        for name in z.files:
            dst = os.path.join(path, name + ".bin")
            a = np.ascontiguousarray(z[name], dtype="<f4")
            data = struct.pack("<i", a.ndim) + struct.pack("<%di" % a.ndim, *a.shape) + a.tobytes()
            if not os.path.exists(dst) or os.path.getsize(dst) != len(data):
                _write_atomic(dst, data)
    return path


def weight_file(model, fp16=False):
    """Path of the staged reference weight file; FileNotFoundError (never a fall-back) when it is not there."""
    key = (model, bool(fp16))
    if key not in FILES:
        raise FileNotFoundError("the reference ships no %s weight file for %s" % ("fp16" if fp16 else "fp32", model))
    path = os.path.join(REF_DIR, "models", FILES[key])
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: build() stages it where the reference tree exists "
                                "(oracle/reference_data.py)" % path)
    return path
