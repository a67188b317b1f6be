"""OpenPose (openpose/model.py:27-141) as an op program."""
import numpy as np

from .. import arch
from .layout import ACT_NONE, ACT_RELU, MODEL_OPENPOSE, OP_COPYCH, OP_MAXPOOL
from .program import Program

# Concat tensor channel layout (192): feat 0..127 | PAF 128..165 (+2 zero) | HM 168..186 (+5 zero).
OP_FEAT, OP_PAF, OP_HM, OP_XCH = 0, 128, 168, 192


def pack_openpose(sd, precision='f32'):
    """openpose/model.py:27-141.  Stage inputs cat[PAF, HM, feat] live in two ping-pong
    192-channel tensors; every stage-output conv writes its slice directly."""
    if precision in ('f16', 'f16x2'):   # the embedder's tolerance modes are for networks without discrete decisions: pose keeps 22 bits
        precision = 'f16x3'
    P = Program(MODEL_OPENPOSE, precision)
    t = P.tensor(4, 1, name='input')
    P.input_tensor = t
    P.input_stats = (np.array([-0.05, -0.05, -0.05, 0.0]), np.array([0.08, 0.08, 0.08, 0.0]))   # RGB / 255 - 0.5 of natural images
    X0 = P.tensor(OP_XCH, 3, name='X0')
    X1 = P.tensor(OP_XCH, 3, name='X1')
    items = arch.OPENPOSE_MODEL0
    skip_pool = False
    for i, item in enumerate(items):
        nxt = items[i + 1] if i + 1 < len(items) else None
        if item[0] == 'pool':
            if skip_pool:                                           # already done in the previous conv's epilogue
                skip_pool = False
                continue
            o = P.tensor(P.tensors[t][0], 1)
            P.simple(OP_MAXPOOL, t, o)
            t = o
            continue
        name, cin, cout, k = item
        W, b = sd['model0.%s.weight' % name], sd['model0.%s.bias' % name]
        if nxt is None:       # conv4_4_CPM -> feature slice of X0
            P.conv(t, X0, W, b, act=ACT_RELU, out_ch_off=OP_FEAT)
            P.tap('feat', X0, OP_FEAT, 128)
        elif nxt[0] == 'pool' and cin % 32 == 0 and cout % 64 == 0:
            # conv + ReLU + 2x2 max-pool in one launch: the full-resolution map (493 MB per 32 frames after conv1_2 at
            # 184 x 327) is never written; max commutes with nothing here -- it is applied to the very values the
            # separate pool would have read
            o = P.tensor(cout, 1, name=name + '_pooled')
            P.conv(t, o, W, b, act=ACT_RELU, pool=True)
            t = o
            skip_pool = True
        else:
            o = P.tensor(cout, 0 if nxt[0] == 'pool' else 1, name=name)
            P.conv(t, o, W, b, act=ACT_RELU)
            t = o
    P.simple(OP_COPYCH, X0, X1, OP_FEAT, OP_FEAT, 128)

    # true input channel (cat order PAF38, HM19, feat128) -> position in the 192-channel tensor
    cat_pos = np.concatenate([OP_PAF + np.arange(38), OP_HM + np.arange(19), OP_FEAT + np.arange(128)])
    for st in range(1, 7):
        xin, xout = (X0, X1) if st % 2 == 1 else (X1, X0)
        # The first conv of the PAF branch and of the heat-map branch read the same stage input with the same
        # kernel size: one launch with their output channels side by side (128 | 128); each branch then goes on
        # from its channel slice.  Per output channel the arithmetic is unchanged.
        l1, l2 = arch.openpose_stage_layers(st, 1), arch.openpose_stage_layers(st, 2)
        (n1, cin, c1, k, r1), (n2, cin2, c2, k2, r2) = l1[0], l2[0]
        assert (cin, k, r1) == (cin2, k2, r2) and c1 == c2 == 128
        W = np.concatenate([np.asarray(sd['model%d_%d.%s.weight' % (st, br, n)]) for br, n in ((1, n1), (2, n2))])
        b = np.concatenate([np.asarray(sd['model%d_%d.%s.bias' % (st, br, n)]) for br, n in ((1, n1), (2, n2))])
        kw = dict(ch_pos=cat_pos, cin_p=OP_XCH) if cin == 185 else dict(in_ch_off=OP_FEAT)   # stage 1: feature slice only
        cur = P.tensor(c1 + c2, l1[1][3] // 2)
        P.conv(xin, cur, W, b, act=ACT_RELU if r1 else ACT_NONE, **kw)
        # The middle layers of the two branches have identical shapes (model.py:56-86): each pair runs as ONE grouped
        # conv (groups=2) over the side-by-side 128 | 128 (or 512 | 512) channels -- twice the tiles per launch, which
        # is what lets the 1080p-sized maps use the 128 x 256 tile, and half the launches.
        for li in range(1, len(l1) - 1):
            (na, cin, cout, k, relu), (nb, cin2, cout2, k2, relu2) = l1[li], l2[li]
            assert (cin, cout, k, relu) == (cin2, cout2, k2, relu2) and cin % 32 == 0 and cout % 128 == 0
            W = np.concatenate([np.asarray(sd['model%d_%d.%s.weight' % (st, br, n)]) for br, n in ((1, na), (2, nb))])
            b = np.concatenate([np.asarray(sd['model%d_%d.%s.bias' % (st, br, n)]) for br, n in ((1, na), (2, nb))])
            o = P.tensor(2 * cout, l1[li + 1][3] // 2)
            P.conv(cur, o, W, b, act=ACT_RELU if relu else ACT_NONE, groups=2)
            cur = o
        # Output convs (1x1 -> 38 PAF / 19 heat-map channels, adjacent slices 128..167 | 168..187 of xout).  Where both are
        # linear and narrow (stages 2-5) they run as ONE launch: rows [PAF 38 + 2 zero | HM 19 + 1 zero] over all 2 cin input channels
        # with zero weights on the other branch's half -- exact zeros, so every output keeps its bits.  Stage 6 keeps two
        # launches: its heat-map conv is followed by a ReLU (the reference's `no_relu_layers` typo), its PAF conv is not.
        (np_, cin, co1, k, r1), (nh, cin2, co2, k2, r2) = l1[-1], l2[-1]
        if r1 == r2 and cin == cin2 <= 128:                       # (stage 1: 2 x 512 inputs, no gain)
            Wp, bp = np.asarray(sd['model%d_1.%s.weight' % (st, np_)]), np.asarray(sd['model%d_1.%s.bias' % (st, np_)])
            Wh, bh = np.asarray(sd['model%d_2.%s.weight' % (st, nh)]), np.asarray(sd['model%d_2.%s.bias' % (st, nh)])
            Wm = np.zeros((60, 2 * cin, 1, 1), np.float32)
            bm = np.zeros(60, np.float32)
            Wm[0:co1, :cin], bm[0:co1] = Wp, bp
            Wm[40:40 + co2, cin:], bm[40:40 + co2] = Wh, bh
            P.conv(cur, xout, Wm, bm, act=ACT_RELU if r1 else ACT_NONE, out_ch_off=OP_PAF, cout_p=60)
            P.ops[-1]['macs_per_pixel'] = float((co1 + co2) * cin)          # algorithmic work: the two real convs
        else:
            for br, layers in ((1, l1), (2, l2)):
                name, cin, cout, k, relu = layers[-1]
                key = 'model%d_%d.%s' % (st, br, name)
                off, cp = (OP_PAF, 40) if br == 1 else (OP_HM, 20)
                P.conv(cur, xout, sd[key + '.weight'], sd[key + '.bias'], act=ACT_RELU if relu else ACT_NONE,
                       in_ch_off=(br - 1) * cin, out_ch_off=off, cout_p=cp)
        P.tap('stage%d_paf' % st, xout, OP_PAF, 38)
        P.tap('stage%d_hm' % st, xout, OP_HM, 19)
    P.outputs = [X0]
    P.tap('pafs', X0, OP_PAF, 38)
    P.tap('heatmaps', X0, OP_HM, 19)
    return P
