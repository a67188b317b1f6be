"""ArcFace (arcface/model.py:4-97) as an op program."""
import numpy as np

from .. import arch
from .batchnorm import _bn_affine, _fold
from .layout import ACT_PRELU, MODEL_ARCFACE
from .program import Program


def pack_arcface(sd, precision='f32'):
    """arcface/model.py:4-97.  The residual stream R is the only tensor between units (halo 1).  A unit opens with a
    BatchNorm in front of a zero-padded 3x3 conv (model.py:12-14): folding it into that conv is exact away from the border
    only -- padded taps are true zeros, not BN(0) -- so the conv gets NINE biases, one per border class of the output pixel
    (Program.conv(in_affine=...)); no BatchNorm'd copy of R is ever stored."""
    eps = arch.ARC_BN_EPS
    P = Program(MODEL_ARCFACE, precision)
    tin = P.tensor(4, 1, name='input')
    P.input_tensor = tin
    P.input_stats = (np.array([-0.1, -0.1, -0.1, 0.0]), np.array([0.25, 0.25, 0.25, 0.0]))      # (BGR - 127.5) / 128 of face crops
    units = list(arch.arcface_units())

    def next_bn(i):
        if i < len(units):
            st, u = units[i][0], units[i][1]
            return _bn_affine(sd, 'stages.%d.%d.body.0' % (st, u), eps)
        return _bn_affine(sd, 'final_layer.0', eps)

    s, sh = _bn_affine(sd, 'initial_layer.1', eps)
    W, b = _fold(sd['initial_layer.0.weight'], None, s, sh)
    R = P.tensor(64, 1, name='stem')
    P.conv(tin, R, W, b, act=ACT_PRELU, prelu=sd['initial_layer.2.weight'])
    for i, (st, u, cin, cout, stride, sc) in enumerate(units):
        p = 'stages.%d.%d' % (st, u)
        s, sh = _bn_affine(sd, p + '.body.2', eps)
        W1, b1 = _fold(sd[p + '.body.1.weight'], None, s, sh)
        Y = P.tensor(cout, 1)
        # stage 4 (7 x 7 maps, 512 channels): 100 output tiles at 64 crops on 256 CUs, 144 K slabs -> K in two fixed halves
        ks = 2 if cout == 512 else 0
        P.conv(R, Y, W1, b1, act=ACT_PRELU, prelu=sd[p + '.body.3.weight'], k_split=ks if cin == 512 else 0,
               in_affine=next_bn(i))
        if sc:
            s, sh = _bn_affine(sd, p + '.shortcut.1', eps)
            Ws, bs = _fold(sd[p + '.shortcut.0.weight'], None, s, sh)
            S = P.tensor(cout, 0)
            P.conv(R, S, Ws, bs, stride=stride, pad=0)
            res = S
        else:
            res = R
        s, sh = _bn_affine(sd, p + '.body.5', eps)
        W2, b2 = _fold(sd[p + '.body.4.weight'], None, s, sh)
        last = i == len(units) - 1
        Rn = P.tensor(cout, 0 if last else 1)
        P.conv(Y, Rn, W2, b2, stride=stride, res=res, k_split=ks)
        if u == arch.ARC_UNITS[st] - 1:
            P.tap('stage%d' % (st + 1), Rn, 0, cout)
        R = Rn
    # head: BN2d -> Flatten(C,H,W) -> Linear -> BN1d, as a 1x1 conv over the (N,1,1,25088) NHWC view
    s, sh = _bn_affine(sd, 'final_layer.4', eps)
    Wl = np.asarray(sd['final_layer.3.weight'], np.float64) * s[:, None]
    bl = np.asarray(sd['final_layer.3.bias'], np.float64) * s + sh
    f = np.arange(7 * 7 * 512)
    ch_pos = (f % 49) * 512 + f // 49
    # no padding between final_layer.0 and the Linear: that BatchNorm folds into the Linear exactly
    s0, t0 = next_bn(len(units))
    chan = f // 49                                              # flatten order (C, H, W): feature f belongs to channel f // 49
    bl = bl + Wl @ t0[chan]
    Wl = Wl * s0[chan][None, :]
    A = P.tensor(7 * 7 * 512, 0, alias_of=R)
    E = P.tensor(512, 0, name='embedding', f32=True)
    # f16 mode: 392 slabs of 64 channels -- below the library's own K-split rule (>= 512 slabs), same 32 ranges asked for here
    P.conv(A, E, Wl.reshape(512, 7 * 7 * 512, 1, 1), bl, ch_pos=ch_pos, pad=0, k_split=32 if P.prec == 4 else 0)
    P.outputs = [E]
    return P
