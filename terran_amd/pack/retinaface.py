"""RetinaFace (retinaface/model.py:53-316) as an op program."""
import os

import numpy as np

from .. import arch
from .batchnorm import _bn_affine, _fold
from .layout import ACT_RELU, MODEL_RETINAFACE
from .program import Program


# Context tensor channel layout (96): ctx3x3 0..31 | reducer 32..47 | ctx5x5 48..63 | 7x7-mid 64..79 |
# ctx7x7 80..95; the merged head conv reads all 96 with zero weights on reducer / 7x7-mid.
def pack_retinaface(sd, precision='f32', fused=None):
    """retinaface/model.py:53-316.  Sibling convs that share an input are merged (ctx3x3+reducer,
    ctx5x5+ctx7x7.0, cls+bbox+landmark heads); the FPN nearest-x2 upsample + add is the
    residual of the lateral 1x1 conv's epilogue.  fused (default in the parity modes): the MobileNet base runs as
    one front kernel (frames -> conv3x3 s2 -> dw3x3 -> 1x1) followed by 12 [depthwise 3x3 -> 1x1] blocks whose depthwise
    output never leaves the CU (27 launches and a float copy of the frames become 13 launches);
    fused=False keeps the layer-by-layer program (the `stem` debug tap; the `bf16` throughput mode)."""
    # The detector's outputs are decisions (score >= 0.5, IoU > 0.4, descending-score ORDER among ~10^2 near-equal
    # scores per image): measured over 208 frames, bf16x3 convs (2^-16 per product) kept every detection but swapped the
    # order of near-tied scores in 3 % of the images.  The graph is HBM-bound (35 FLOP/B), so the exact-f32 MFMA costs
    # next to nothing here: in the `bf16x3` mode the detector runs on it, and its results ARE the `f32` mode's, bit for
    # bit.  (`bf16`, the throughput mode outside the parity bar, stays bf16.)  All activations are float32.
    if precision in ('f16', 'f16x2'):   # the embedder's tolerance modes are for networks without discrete decisions: the detector keeps 22 bits
        precision = 'f16x3'
    det_prec = 'f32' if precision in ('bf16x3', 'f16x3') else precision
    P = Program(MODEL_RETINAFACE, det_prec)
    # f16x3: the REFINER (FPN laterals, 3x3 aggregations, context modules, heads: 18 dense convs, 0.75 of the detector's
    # 1.5 ms at C2 and f32-MFMA-bound) runs on the split-half MFMA -- 22-bit operands, measured 0 decision flips / order
    # swaps against the oracle over 224 frames, the same as exact f32 (bf16x3's 16 bits swapped near-tied scores in 3 % of
    # the images: that mode keeps the whole detector exact f32).  The MobileNet base stays exact f32: its input is raw
    # 0..255 pixels and it is bound by its depthwise taps, not by the matrix pipe.
    refiner_prec = 'f16x3' if precision == 'f16x3' else None
    P.allow_split = refiner_prec is not None
    if fused is None:
        fused = P.prec == 0
    tin = P.tensor(4, 1, alias_of=-2 if fused else -1, name='input')
    P.input_tensor = tin
    P.input_stats = (np.array([110.0, 110.0, 110.0, 0.0]), np.array([4900.0, 4900.0, 4900.0, 0.0]))   # raw 0..255 BGR pixels
    eps = arch.RETINA_BASE_BN_EPS

    def cbr(key_conv, key_bn, e=eps, bias=False):
        s, sh = _bn_affine(sd, key_bn, e)
        return _fold(sd[key_conv + '.weight'], sd[key_conv + '.bias'] if bias else None, s, sh)

    # the base network as a chain: stem conv, then alternating depthwise / pointwise layers
    pw_keys = [('base.scales.%d.%d.conv_block.0' % (si, bi), 'base.scales.%d.%d.conv_block.1' % (si, bi), cout, both)
               for si, scale in enumerate(arch.RETINA_SCALES) for bi, (cin, cout, stride, both) in enumerate(scale)]
    pw_keys += [('base.final_conv.0.conv_block.0', 'base.final_conv.0.conv_block.1', 256, False),
                ('base.final_conv.1', 'base.final_conv.2', 256, True)]
    dw_keys = [('base.first_conv_block.3', 'base.first_conv_block.4', 1)]
    dw_keys += [('base.scales.%d.%d.sep_block.0' % (si, bi), 'base.scales.%d.%d.sep_block.1' % (si, bi), stride)
                for si, scale in enumerate(arch.RETINA_SCALES) for bi, (cin, cout, stride, both) in enumerate(scale)]
    dw_keys += [('base.final_conv.0.sep_block.0', 'base.final_conv.0.sep_block.1', 1)]
    assert len(pw_keys) == len(dw_keys) == 13
    feats = []
    if fused:
        Ws, bs = cbr('base.first_conv_block.0', 'base.first_conv_block.1')
        t = None
        # the front kernel also runs the next block (depthwise stride 2 -> 1x1 16 -> 32): the 16-channel half-resolution map stays
        # on the CU (TERRAN_AMD_NO_FUSED_FRONT: the two as separate launches, A/B)
        fuse_front = not os.environ.get('TERRAN_AMD_NO_FUSED_FRONT')
        front = None
        for i, ((dk, dbn, stride), (pk, pbn, cout, both)) in enumerate(zip(dw_keys, pw_keys)):
            Wd, bd = cbr(dk, dbn)
            Wp, bp = cbr(pk, pbn)
            if i == 0 and fuse_front:
                front = (Wd, bd, Wp, bp)
                continue
            c = P.tensor(cout, 1 if i < 12 else 0)
            if i == 0:
                P.rfstem(tin, c, Ws, bs, Wd, bd, Wp, bp)
            elif i == 1 and front is not None:
                assert stride == 2 and cout == 32 and Wd.shape[0] == 16 and not both
                P.rfstem(tin, c, Ws, bs, *front, Wd, bd, Wp, bp)
            else:
                # the 1x1 of a [depthwise -> pointwise] block follows the refiner's mode from the stride-8 maps on (cin >= 64):
                # the two blocks on the 104 x 185 maps are bound by their depthwise taps and stay exact f32
                P.dwpw(t, c, Wd, bd, Wp, bp, stride=stride, precision=refiner_prec if Wd.shape[0] >= 64 else None)
            if both:
                feats.append(c)
            t = c
    else:
        W, b = cbr('base.first_conv_block.0', 'base.first_conv_block.1')
        a0 = P.tensor(8, 1)
        P.conv(tin, a0, W, b, stride=2, act=ACT_RELU)
        t = a0
        for i, ((dk, dbn, stride), (pk, pbn, cout, both)) in enumerate(zip(dw_keys, pw_keys)):
            W, b = cbr(dk, dbn)
            d = P.tensor(P.tensors[t][0], 0, name='stem' if i == 0 else None)
            P.dwconv(t, d, W, b, stride=stride)
            W, b = cbr(pk, pbn)
            c = P.tensor(cout, 1 if i < 12 else 0)
            P.conv(d, c, W, b, act=ACT_RELU)
            if both:
                feats.append(c)
            t = c
    f8, f16, f32 = feats
    P.tap('feat8', f8, 0, 64)
    P.tap('feat16', f16, 0, 128)
    P.tap('feat32', f32, 0, 256)

    e2 = arch.RETINA_REFINER_BN_EPS
    rp = refiner_prec

    def rcbr(p):
        return cbr(p + '.0', p + '.1', e2, bias=True)

    A = arch.RETINA_NUM_ANCHORS
    heads = {}
    # The context module + heads of a pyramid level depend on that level's map only.  The stride-32 and stride-16 levels are
    # 4 launches of 9-22 us each (a few dozen tiles: launch latency, not work): they go to side streams ("lanes") right
    # behind the op that finishes their map and run beside the rest of the refiner instead of in front of it.
    use_lanes = not os.environ.get('TERRAN_AMD_NO_DETECTOR_LANES')

    def context_and_heads(s, x, lane):
        P.lane = lane if use_lanes else 0
        p = 'refiner.context_stride%d' % s
        ctx = P.tensor(96, 1)
        W3, b3 = rcbr(p + '.context_3x3')
        Wr, br_ = rcbr(p + '.dimension_reducer')
        P.conv(x, ctx, np.concatenate([W3, Wr]), np.concatenate([b3, br_]), act=ACT_RELU, out_ch_off=0, precision=rp)
        W5, b5 = rcbr(p + '.context_5x5')
        W7, b7 = cbr(p + '.context_7x7.0', p + '.context_7x7.1', e2, bias=True)
        P.conv(ctx, ctx, np.concatenate([W5, W7]), np.concatenate([b5, b7]), act=ACT_RELU, in_ch_off=32,
               out_ch_off=48, precision=rp)
        W7b, b7b = cbr(p + '.context_7x7.3', p + '.context_7x7.4', e2, bias=True)
        P.conv(ctx, ctx, W7b, b7b, act=ACT_RELU, in_ch_off=64, out_ch_off=80, precision=rp)
        P.tap('ctx%d_3x3' % s, ctx, 0, 32)
        P.tap('ctx%d_5x5' % s, ctx, 48, 16)
        P.tap('ctx%d_7x7' % s, ctx, 80, 16)
        # merged heads: rows [cls 2A | bbox 4A | landmark 10A]; input order cat[3x3, 5x5, 7x7]
        Wh = np.concatenate([sd['outputs.%s_stride%d.weight' % (h, s)] for h in ('cls', 'bbox', 'landmark')])
        bh = np.concatenate([sd['outputs.%s_stride%d.bias' % (h, s)] for h in ('cls', 'bbox', 'landmark')])
        pos = np.concatenate([np.arange(32), 48 + np.arange(16), 80 + np.arange(16)])
        hd = P.tensor(16 * A, 0, name='head%d' % s, f32=True)
        P.conv(ctx, hd, Wh, bh, ch_pos=pos, cin_p=96, precision=rp)
        heads[s] = hd
        P.lane = 0

    W, b = rcbr('refiner.conv_stride32')
    p32 = P.tensor(64, 1, name='p32')
    P.conv(f32, p32, W, b, act=ACT_RELU, precision=rp)
    context_and_heads(32, p32, 1)
    W, b = rcbr('refiner.conv_stride16')
    s16 = P.tensor(64, 1)
    P.conv(f16, s16, W, b, act=ACT_RELU, res=p32, res_up2=1, precision=rp)
    W, b = rcbr('refiner.aggr_stride16')
    p16 = P.tensor(64, 1, name='p16')
    P.conv(s16, p16, W, b, act=ACT_RELU, precision=rp)
    context_and_heads(16, p16, 2)
    W, b = rcbr('refiner.conv_stride8')
    s8 = P.tensor(64, 1)
    P.conv(f8, s8, W, b, act=ACT_RELU, res=p16, res_up2=1, precision=rp)
    W, b = rcbr('refiner.aggr_stride8')
    p8 = P.tensor(64, 1, name='p8')
    P.conv(s8, p8, W, b, act=ACT_RELU, precision=rp)
    context_and_heads(8, p8, 0)
    P.outputs = [heads[32], heads[16], heads[8]]
    return P
