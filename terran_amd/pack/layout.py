"""What a packed program looks like in bytes: the constants, the header / tensor / op records of the blob (they mirror
`terran_amd/csrc/ta_internal.h`: ta_blob_header / ta_tensor_desc / ta_op_desc), the weight region, and the row formats of the
weight images ([K-slab][cout][32 floats], split into bf16 / half-float hi | lo pairs where the arithmetic mode wants it)."""
import numpy as np

MODEL_RETINAFACE, MODEL_ARCFACE, MODEL_OPENPOSE = 1, 2, 3
OP_CONV, OP_DWCONV, OP_MAXPOOL, OP_COPYCH, OP_RFSTEM, OP_DWPW = 1, 2, 3, 4, 5, 6
ACT_NONE, ACT_RELU, ACT_PRELU = 0, 1, 2
MAGIC = 0x314D4154

HEADER_DT = np.dtype({
    'names': ['magic', 'version', 'kind', 'n_tensors', 'n_ops', 'input_tensor', 'n_outputs', 'outputs',
              'tensors_off', 'ops_off', 'weights_off', 'weights_bytes'],
    'formats': ['<u4', '<u4', '<i4', '<i4', '<i4', '<i4', '<i4', ('<i4', 16), '<i8', '<i8', '<i8', '<i8'],
    'offsets': [0, 4, 8, 12, 16, 20, 24, 28, 96, 104, 112, 120],
    'itemsize': 128,
})
TENSOR_DT = np.dtype([('channels', '<i4'), ('halo', '<i4'), ('alias_of', '<i4'), ('fmt', '<i4'), ('unscale_off', '<i4')])
FMT_F32, FMT_SPLIT, FMT_SPLIT16, FMT_F16 = 0, 1, 2, 3
_OP_I32 = ['type', 'in', 'out', 'in_ch_off', 'cin', 'out_ch_off', 'cout', 'coutp', 'kh', 'kw', 'stride', 'pad',
           'act', 'res', 'res_ch_off', 'res_up2', 'out2', 'out2_ch_off', 'n_slabs', 'prec', 'groups', 'variant', 'pool', 'wscale_log2']
_OP_I64 = ['w_off', 'bias_off', 'prelu_off', 'scale2_off', 'shift2_off', 'wus_off']
OP_DT = np.dtype([(n, '<i4') for n in _OP_I32] + [(n, '<i8') for n in _OP_I64] + [('macs_per_pixel', '<f8')])
assert OP_DT.itemsize == 152 and TENSOR_DT.itemsize == 20
BLOB_VERSION = 9            # 9: OP_RFSTEM with cout == 32 = the front kernel fused with the next depthwise + 1x1 block; 8: per-channel activation scales (ta_tensor_desc.unscale_off) and per-output-channel un-scale vectors (ta_op_desc.wus_off) replace the per-layer wscale_log2; 7: arithmetic mode 4 ('f16') and the 2-byte tensor format; 6: op lanes (variant bits 17..18); 2: ta_op_desc grew `groups` (grouped convs); 3: fused RetinaFace ops (OP_RFSTEM, OP_DWPW), `variant`; 4: `pool`; 5: `wscale_log2` (f16x3)

PRECISIONS = {'f32': 0, 'bf16x3': 1, 'bf16': 2, 'f16x3': 3, 'f16': 4, 'f16x2': 5}     # 'f16x2': f16x3's tensors and weights, two of its three MFMAs per product ((w_hi + w_lo) * x_hi): embedder only
SPLIT_FMT = {0: FMT_F32, 1: FMT_SPLIT, 2: FMT_SPLIT, 3: FMT_SPLIT16, 4: FMT_F16, 5: FMT_SPLIT16}     # pre-split activation format per arithmetic mode

# ta_op_desc fields an op type leaves alone; `op_desc` fills in the rest
_OP_DEFAULTS = dict(in_ch_off=0, out_ch_off=0, coutp=0, kh=1, kw=1, stride=1, pad=0, act=ACT_NONE, res=-1, res_ch_off=0, res_up2=0,
                    out2=-1, out2_ch_off=0, n_slabs=0, prec=0, groups=1, variant=0, pool=0, wscale_log2=0,       # wscale_log2: dead since blob version 8
                    w_off=-1, bias_off=-1, prelu_off=-1, scale2_off=-1, shift2_off=-1, wus_off=-1, macs_per_pixel=0.0)


def op_desc(typ, tin, tout, cin, cout, **fields):
    """One ta_op_desc as a dict with every field of OP_DT: the defaults above, then what the caller says differs."""
    op = dict(_OP_DEFAULTS, type=typ, out=tout, cin=cin, cout=cout, **fields)
    op['in'] = tin
    assert set(op) == set(OP_DT.names), set(op) ^ set(OP_DT.names)
    return op


def _rup(x, m):
    return (x + m - 1) // m * m


class WeightRegion:
    """The blob's weight region: chunks of float32 (or raw bytes) at 256-byte aligned offsets, in the order they are asked for.
    A chunk may be reserved first and filled later, or rewritten at the same size."""

    def __init__(self):
        self.chunks = []       # bytes (None: reserved, not yet filled), each followed by its padding
        self.nbytes = 0
        self._at = {}          # offset -> (index into chunks, size)

    def reserve(self, nbytes, data=None):
        off, nbytes = self.nbytes, int(nbytes)
        self._at[off] = (len(self.chunks), nbytes)
        self.chunks.append(data)
        pad = -nbytes % 256
        if pad:
            self.chunks.append(b'\0' * pad)
        self.nbytes += nbytes + pad
        return off

    def add(self, arr):
        data = np.ascontiguousarray(arr, dtype=np.float32).tobytes()
        return self.reserve(len(data), data)

    def rewrite(self, off, data):
        """Fill or replace the chunk at `off` (same size); `data`: bytes, or an array stored as float32."""
        if not isinstance(data, bytes):
            data = np.ascontiguousarray(data, dtype=np.float32).tobytes()
        k, size = self._at[off]
        assert len(data) == size, (len(data), size)
        self.chunks[k] = data

    def tobytes(self):
        return b''.join(self.chunks)


def _bf16_bits(x):
    """float32 -> bfloat16 bit pattern (uint16), round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def _bf16_to_f32(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def split_bf16_rows(packed):
    """[slab][cout][32] float32 -> the same 128-byte rows as [hi x32 | lo x32] bfloat16, returned as a
    float32-typed view of the bytes (x = hi + lo to ~2^-17 relative)."""
    hi = _bf16_bits(packed)
    lo = _bf16_bits(packed - _bf16_to_f32(hi))
    rows = np.concatenate([hi, lo], axis=-1)                # (..., 64) uint16
    return np.ascontiguousarray(rows).view(np.float32)      # (..., 32)


def row_exponents(packed):
    """[slab][cout][32] float32 -> per-output-channel exponents s[cout]: max |W[co, :]| 2^s[co] lies in [2^13, 2^14)
    (0 for an all-zero row)."""
    m = np.abs(np.asarray(packed, np.float32)).max(axis=(0, 2)).astype(np.float64)
    ok = np.isfinite(m) & (m > 0)
    s = np.zeros(m.shape, np.int64)
    s[ok] = np.clip(13 - np.floor(np.log2(m[ok])), -60, 60).astype(np.int64)
    return s


def split_f16_rows(packed, exps=None):
    """[slab][cout][32] float32 -> ([hi x32 | lo x32] IEEE half rows viewed as float32, exponents s[cout]).

    Half floats carry 11 significant bits down to 2^-14 only; a lo half below that loses bits.  Every OUTPUT CHANNEL's
    row is therefore packed times 2^s[co], s[co] chosen so that max |W[co, :]| 2^s[co] lies in [2^13, 2^14): every weight
    within 2^-16 of its row's largest keeps a normal lo half (22 significant bits in hi + lo), nothing gets near 65504,
    and a channel whose weights are all small (a BatchNorm with a small gamma / sigma folded in) keeps its bits instead of
    inheriting the scale of the layer's largest channel.  The conv epilogue multiplies the sums by 2^-s[co] (folded into
    its per-channel un-scale vector, program.py: _rewrite_bias), which is exact."""
    packed = np.ascontiguousarray(packed, dtype=np.float32)
    s = row_exponents(packed) if exps is None else np.asarray(exps, np.int64)
    scaled = np.ldexp(packed, s[None, :, None].astype(np.int32)).astype(np.float32)               # exact (powers of two)
    hi = scaled.astype(np.float16)
    lo = (scaled - hi.astype(np.float32)).astype(np.float16)
    rows = np.concatenate([hi.view(np.uint16), lo.view(np.uint16)], axis=-1)
    return np.ascontiguousarray(rows).view(np.float32), s


def pack_rows(flat, coutp, prec):
    """(n_slabs * 32, coutp) float32 weights, K down the rows -> the [slab][cout][32] image the kernels read, split into
    half floats / bf16 where arithmetic mode `prec` wants it.  -> (bytes, row exponents s[coutp]: 0 outside the half-float modes)."""
    packed = np.ascontiguousarray(flat.reshape(flat.shape[0] // 32, 32, coutp).transpose(0, 2, 1))
    wexp = np.zeros(coutp, np.int64)
    if prec in (3, 4, 5):
        packed, wexp = split_f16_rows(packed)
    elif prec != 0:
        packed = split_bf16_rows(packed)
    return np.ascontiguousarray(packed, dtype=np.float32).tobytes(), wexp


def fold_input_affine(W, bias, scale, shift):
    """conv3x3(pad0(scale * x + shift)) + bias  ==  conv3x3(pad0(x); W') + bias16[class of the output pixel].

    The scale folds into the weights; the shift reaches an output only through the taps that are not padding, so it becomes
    one bias per border class: per axis the pixel is the first / a middle / the last / the ONLY row (column), class =
    4 * cy + cx (csrc/conv_igemm.hip: ta_border_class), 5 = interior.  W (cout, cin, 3, 3) float64 -> (W', bias16 (16, cout))."""
    W = np.asarray(W, np.float64)
    a_s, a_t = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    T = np.einsum('ocyx,c->oyx', W, a_t)                                  # what the shift adds through tap (ky, kx)
    b0 = np.zeros(W.shape[0]) if bias is None else np.asarray(bias, np.float64)
    valid = ([1, 2], [0, 1, 2], [0, 1], [1])                              # in-bounds taps of a first / middle / last / only row or column
    bias16 = np.stack([b0 + T[:, valid[cy]][:, :, valid[cx]].sum((1, 2)) for cy in range(4) for cx in range(4)])
    return W * a_s[None, :, None, None], bias16
