"""Pack a Terran `state_dict` into the op program + weight blob `libterran_amd.so` runs.

Replaces the reference's `load_model()` + `nn.Module` construction
(retinaface/wrapper.py:16-22, arcface/wrapper.py:13-19, openpose/wrapper.py:27-36):
BatchNorms are folded (float64 math, float32 result), weights are laid out for the
implicit-GEMM kernel ([K-slab][cout][32 floats], K = (ky,kx,cin) with cin fastest), and
the graph is flattened into conv / depthwise / pool / copy ops over halo-padded NHWC
tensors.  Concats become channel slices of a shared tensor; the few graph-level fusions
(merged sibling convs, residual/upsample-add and the next unit's BatchNorm in the conv
epilogue) are documented next to each builder.

    layout.py      constants, the blob's records (they mirror `terran_amd/csrc/ta_internal.h`), weight region, row formats
    moments.py     expected (mean, variance, bound) per channel: what the activation scales of the half-float modes come from
    program.py     `Program`: op emitters, the blob, the repack cache file
    storage.py     per tensor: storage format and the exponents its channels are stored with
    batchnorm.py   BatchNorm folding
    openpose.py, arcface.py, retinaface.py     one network's packer each
    switches.py    the environment switches the packers read, the hash of these sources
"""
from .arcface import pack_arcface
from .layout import (ACT_NONE, ACT_PRELU, ACT_RELU, BLOB_VERSION, FMT_F16, FMT_F32, FMT_SPLIT, FMT_SPLIT16, HEADER_DT, MAGIC,    # noqa: F401
                     MODEL_ARCFACE, MODEL_OPENPOSE, MODEL_RETINAFACE, OP_CONV, OP_COPYCH, OP_DT, OP_DWCONV, OP_DWPW, OP_MAXPOOL,
                     OP_RFSTEM, PRECISIONS, SPLIT_FMT, TENSOR_DT, fold_input_affine, row_exponents, split_bf16_rows, split_f16_rows)
from .moments import _ACT_TARGET_LOG2, _CH_SPREAD, act_moments    # noqa: F401  (the values at import: experiments assign them on `moments`)
from .openpose import pack_openpose
from .program import Program    # noqa: F401
from .retinaface import pack_retinaface
from .switches import PACK_SWITCHES, active_switches, source_tag    # noqa: F401

PACKERS = {MODEL_RETINAFACE: pack_retinaface, MODEL_ARCFACE: pack_arcface, MODEL_OPENPOSE: pack_openpose}
