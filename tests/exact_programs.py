"""Small op programs whose right answer is ONE bit pattern, and their float64 reference (no GPU import).

The HBM-bound layer kernels (csrc/layers.hip: preprocess, depthwise 3x3, 2x2 max-pool, channel-slice copy, the RetinaFace
front) and the format helpers they go through (csrc/act_format.h: ta_ld4 / ta_st4 / ta_ld1) move and combine numbers; on
inputs whose values and partial sums are exactly representable in every storage format there is nothing to round, so a
tolerance has nothing to forgive: any mistake in addressing, format or exponent changes the bits.

The rule (`reference` asserts it, DESIGN.md states it): every value a program holds and every partial sum of the products
that make it is an integer of at most 16 significant bits -- what a bf16 hi + lo pair carries (the half-float pair carries
22) -- and at most 65504, the end of the half-float range for the tensors the packer stores unscaled.  A tensor that is
only ever held as float32 (pinned f32 and read by no op, or inside the all-float32 front kernel) may reach 2^24.  The
bound is taken over sum |w| |x| + |b|, so it holds for every summation order a kernel may choose.  Through a conv's output stage
it is carried on: times max(1, |slope|) of an integer PReLU slope, plus |shortcut|, and times |scale2| plus |shift2| (integers)
into the second output, each against the limit of the tensor it lands in.

Every program is of kind MODEL_RETINAFACE unless said otherwise: its preprocess writes BGR integers 0..255 as float32, 4th
channel 0, into the tensor named 'input'.  A SELECTOR conv (1x1 or 3x3, integer weights and bias) turns that into an exactly
known C-channel tensor in whatever format the packer picks; the ops under test read it.
"""
import numpy as np

from terran_amd import pack

LIMIT_SPLIT = 1 << 16          # 16 significant bits: bf16 hi + lo
LIMIT_F32 = 1 << 24
F16_MAX = 65504.0
PINNED_EXPONENT = -1

# moments of uniform 0..255 pixels (the packer derives the activation exponents of the half-float modes from these)
PIXEL_STATS = (np.array([127.5] * 3 + [0.0]), np.array([(256.0 ** 2 - 1.0) / 12.0] * 3 + [0.0]))


def frames(seed, n, h, w):
    """(n, h, w, 3) uint8 RGB; every byte value occurs as soon as the batch has 256 bytes."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, n * h * w * 3, dtype=np.uint8)
    if f.size >= 256:
        f[rng.permutation(f.size)[:256]] = np.arange(256, dtype=np.uint8)
    return f.reshape(n, h, w, 3)


# ---- integer weights ------------------------------------------------------------------------------------------------------------
def selector_weights(rng, cout, k=1, wmax=64, cin=3, density=1.0):
    """(cout, cin, k, k) integer weights and integer bias.  Channel magnitudes step down by 4 (wmax, wmax / 4, ...: a wrong
    pixel in a weak channel is small against the tensor's largest value); channel c % 8 == 5 has no positive weight and a
    negative bias (all-negative windows when no ReLU follows)."""
    mag = np.maximum(1, wmax >> (2 * (np.arange(cout) % 4)))
    W = rng.integers(-1000, 1001, (cout, cin, k, k)) % (2 * mag[:, None, None, None] + 1) - mag[:, None, None, None]
    if density < 1.0:
        W = W * (rng.random(W.shape) < density)
    b = rng.integers(-1000, 1001, cout) % (2 * 8 * mag + 1) - 8 * mag
    neg = np.arange(cout) % 8 == 5
    W[neg] = -np.abs(W[neg])
    b[neg] = -np.abs(b[neg]) - 1
    return W.astype(np.float64), b.astype(np.float64)


def dw_weights(rng, C, center=2):
    """(C, 1, 3, 3) taps in {-1, 0, 1}, centre tap +-`center`: sum |w| <= 8 + center; integer bias."""
    W = rng.integers(-1, 2, (C, 1, 3, 3))
    W[:, 0, 1, 1] = center * rng.choice([-1, 1], C)
    return W.astype(np.float64), rng.integers(-50, 51, C).astype(np.float64)


def sparse_weights(rng, shape, nonzero, values=(-1, 1, 1, 1), bias=20):
    """Integer weights of `shape` (cout first) with `nonzero` entries per output channel drawn from `values`; integer bias."""
    cout = shape[0]
    W = np.zeros((cout, int(np.prod(shape[1:]))))
    for o in range(cout):
        W[o, rng.permutation(W.shape[1])[:nonzero]] = rng.choice(values, min(nonzero, W.shape[1]))
    return W.reshape(shape), rng.integers(-bias, bias + 1, cout).astype(np.float64)


# ---- float64 reference ops ------------------------------------------------------------------------------------------------------
def _out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_ref(x, W, b, stride=1, pad=0):
    """x (N, C, H, W) float64, W (O, C, kh, kw), zero padding."""
    O, C, kh, kw = W.shape
    xp = np.pad(x[:, :C], ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ho, wo = _out(x.shape[2], kh, stride, pad), _out(x.shape[3], kw, stride, pad)
    out = np.zeros((x.shape[0], O, max(ho, 0), max(wo, 0)))
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            out += np.moveaxis(np.tensordot(W[:, :, ky, kx], patch, axes=([1], [1])), 0, 1)
    return out + np.asarray(b)[None, :, None, None]


def dw_ref(x, W, b, stride=1):
    """Depthwise 3x3, pad 1.  W (C, 1, 3, 3)."""
    C = W.shape[0]
    xp = np.pad(x[:, :C], ((0, 0), (0, 0), (1, 1), (1, 1)))
    ho, wo = _out(x.shape[2], 3, stride, 1), _out(x.shape[3], 3, stride, 1)
    out = np.zeros((x.shape[0], C, ho, wo))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] * W[None, :, 0, ky, kx, None, None]
    return out + np.asarray(b)[None, :, None, None]


def pool_ref(x):
    """2x2 / 2 max-pool, floor: the last row / column of an odd map is dropped."""
    h2, w2 = x.shape[2] // 2, x.shape[3] // 2
    v = x[:, :, :2 * h2, :2 * w2].reshape(x.shape[0], x.shape[1], h2, 2, w2, 2)
    return v.max(axis=(3, 5))


def input_ref(fr):
    """What the RetinaFace preprocess writes: BGR 0..255, 4th channel 0, NCHW float64."""
    x = np.zeros((fr.shape[0], 4) + fr.shape[1:3])
    x[:, :3] = np.transpose(fr[..., ::-1], (0, 3, 1, 2))
    return x


def _exact(what, bound, limit):
    """`bound`: sum |w| |x| + |b| per output value -- no partial sum, in any order, is larger."""
    top = float(bound.max()) if bound.size else 0.0
    assert top < limit, '%s: partial sums reach %.0f, not exact below %d' % (what, top, limit)


# ---- programs -------------------------------------------------------------------------------------------------------------------
class Net:
    """A pack.Program plus the recipe `reference` replays in float64.  Tensors are addressed by name."""

    def __init__(self, precision, kind=pack.MODEL_RETINAFACE, in_halo=1, shape_only_input=False):
        self.P = P = pack.Program(kind, precision)
        self.precision = precision
        self.tid = {}
        self.steps = []
        self.mid_ops = {}                                         # dst name -> op index of a dw+pw block
        self.conv_ops = {}                                        # dst name -> op index of the last conv that writes it
        t0 = P.tensor(4, in_halo, alias_of=-2 if shape_only_input else -1, name='input')
        self.tid['input'] = t0
        P.input_tensor = t0
        P.input_stats = PIXEL_STATS

    def tensor(self, name, c, halo=0, f32=False):
        self.tid[name] = self.P.tensor(c, halo, name=name, f32=f32)
        return name

    def conv(self, src, dst, W, b, *, stride=1, pad=None, relu=False, pool=False, prelu=None, res=None, res_ch_off=0, res_up2=0,
             out2=None, out2_ch_off=0, scale2=None, shift2=None, out_ch_off=0, in_ch_off=0, cin_p=None, groups=1, k_split=0,
             in_affine=None, variant=0):
        """pack.Program.conv with tensors by name.  The output stage in the kernels' order: conv + bias (in_affine: of scale * x +
        shift, zero-padded AFTER the affine), ReLU / PReLU, + res[:, res_ch_off:+cout, y >> res_up2, x >> res_up2], store into the
        slice at out_ch_off, then out2[:, out2_ch_off:+cout] = out * scale2 + shift2."""
        act = pack.ACT_PRELU if prelu is not None else (pack.ACT_RELU if relu else pack.ACT_NONE)
        tid = lambda n: -1 if n is None else self.tid[n]
        self.conv_ops[dst] = len(self.P.ops)
        self.P.conv(self.tid[src], self.tid[dst], W, b, stride=stride, pad=pad, act=act, pool=pool, prelu=prelu, res=tid(res),
                    res_ch_off=res_ch_off, res_up2=res_up2, out2=tid(out2), out2_ch_off=out2_ch_off, scale2=scale2, shift2=shift2,
                    out_ch_off=out_ch_off, in_ch_off=in_ch_off, cin_p=cin_p, groups=groups, k_split=k_split, in_affine=in_affine,
                    variant=variant)
        self.steps.append(('conv', src, dst, dict(W=W, b=b, stride=stride, pad=W.shape[2] // 2 if pad is None else pad, relu=relu, pool=pool,
                                                  prelu=prelu, res=res, res_ch_off=res_ch_off, res_up2=res_up2, out2=out2,
                                                  out2_ch_off=out2_ch_off, scale2=scale2, shift2=shift2, out_ch_off=out_ch_off,
                                                  in_ch_off=in_ch_off, groups=groups, k_split=k_split, in_affine=in_affine)))

    def dwconv(self, src, dst, W, b, *, stride=1, relu=True):
        self.P.dwconv(self.tid[src], self.tid[dst], W, b, stride=stride, relu=relu)
        self.steps.append(('dwconv', src, dst, dict(W=W, b=b, stride=stride, relu=relu)))

    def maxpool(self, src, dst):
        self.P.simple(pack.OP_MAXPOOL, self.tid[src], self.tid[dst])
        self.steps.append(('maxpool', src, dst, {}))

    def copych(self, src, dst, in_off, out_off, ch):
        self.P.simple(pack.OP_COPYCH, self.tid[src], self.tid[dst], in_ch_off=in_off, out_ch_off=out_off, ch=ch)
        self.steps.append(('copych', src, dst, dict(in_off=in_off, out_off=out_off, ch=ch)))

    def dwpw(self, src, dst, Wd, bd, Wp, bp, *, stride=1):
        self.mid_ops[dst] = len(self.P.ops)
        self.P.dwpw(self.tid[src], self.tid[dst], Wd, bd, Wp, bp, stride=stride)
        self.steps.append(('dwpw', src, dst, dict(Wd=Wd, bd=bd, Wp=Wp, bp=bp, stride=stride)))

    def rfstem(self, dst, blocks):
        """blocks: [(Ws, bs), (Wd, bd, Wp, bp)] or with a third (Wd2, bd2, Wp2, bp2): the fused second block."""
        self.P.rfstem(self.tid['input'], self.tid[dst], *blocks[0], *blocks[1], *(blocks[2] if len(blocks) > 2 else ()))
        self.steps.append(('rfstem', 'input', dst, dict(blocks=blocks)))

    def pin_exponent(self, name, e=PINNED_EXPONENT):
        """Half-float modes: store every channel of tensor `name` times 2^e instead of what the packer would choose per channel,
        so that the exponent of whatever shares its channels (pooled, copied) is visibly the SHARED one and not a second estimate
        that happens to agree.  2^-1 keeps any 16-bit integer inside the half-float range."""
        self.P.forced_scale[self.tid[name]] = e

    def read_by_an_op(self, name):
        t = self.tid[name]
        return any(op['in'] == t or op['res'] == t for op in self.P.ops)

    def limit(self, name):
        """2^24 for a tensor only ever held as float32 (pinned, read by no op), else 16 significant bits."""
        return LIMIT_F32 if self.tid[name] in self.P.f32_only and not self.read_by_an_op(name) else LIMIT_SPLIT


MISTAKES = ('up2_unshifted', 'res_ch_off+4', 'out2_ch_off+8', 'prelu_shifted', 'corner_as_edge', 'k_range_dropped', 'no_shift2')


def border_class(n):
    """Per axis: first 0, middle 1, last 2, the only one 3 (csrc/conv_common.h: ta_border_class; class = 4 cy + cx)."""
    c = np.ones(n, np.int64)
    c[0], c[-1] = 0, 2
    return c if n > 1 else np.array([3])


def k_range_mask(W, k_split, r):
    """True where weight W[o, c, ky, kx] lies in K range `r` of `k_split`: K runs (tap, channel), in slabs of 32, range r is slabs
    [r n / k_split, (r + 1) n / k_split)."""
    _, cin, kh, kw = W.shape
    n = kh * kw * cin // 32
    kidx = np.arange(kh * kw * cin)
    m = (kidx >= r * n // k_split * 32) & (kidx < (r + 1) * n // k_split * 32)
    return m.reshape(kh, kw, cin).transpose(2, 0, 1)[None]


def _conv_step(net, ref, x, dst, a, lim, chans, mistake):
    """One conv of `reference` with its whole output stage.  Returns what `dst` holds afterwards; writes `out2` into ref itself.
    `mistake`: one of MISTAKES (the deliberately wrong references of tests/test_exact_programs_cpu.py), or 'fold': in_affine by the
    packer's folded weights and border-class biases instead of by its meaning."""
    strict = mistake is None
    W, b, g = np.asarray(a['W'], np.float64), np.asarray(a['b'], np.float64), a['groups']
    cout, cin = W.shape[:2]
    xin = x[:, a['in_ch_off']:a['in_ch_off'] + cin * g]
    assert xin.shape[1] == cin * g
    xabs = np.abs(xin)
    if a['k_split'] > 1 and mistake == 'k_range_dropped':
        W = W * ~k_range_mask(W, a['k_split'], 1)
    aff = a['in_affine']
    if aff is not None and mistake in ('fold', 'corner_as_edge'):
        Wf, b16 = pack.fold_input_affine(W, b, *aff)
        y = conv_ref(xin, Wf, np.zeros(cout), 1, 1)
        cy, cx = border_class(y.shape[2]), border_class(y.shape[3])
        cls = 4 * cy[:, None] + cx[None, :]
        if mistake == 'corner_as_edge':
            cls = np.where((cy[:, None] != 1) & (cx[None, :] != 1), 4 * cy[:, None] + 1, cls)
        y = y + np.transpose(b16[cls], (2, 0, 1))[None]
        aff = None
    elif aff is not None:
        sc, sh = (np.asarray(v, np.float64)[None, :, None, None] for v in aff)
        xin, xabs = xin * sc + sh, xabs * np.abs(sc) + np.abs(sh)                       # bounds the folded form as well
    if aff is not None or a['in_affine'] is None:
        cg, og = cin, cout // g
        y = np.concatenate([conv_ref(xin[:, i * cg:(i + 1) * cg], W[i * og:(i + 1) * og], b[i * og:(i + 1) * og], a['stride'], a['pad'])
                            for i in range(g)], axis=1)
    cg, og = cin, cout // g
    bound = np.concatenate([conv_ref(xabs[:, i * cg:(i + 1) * cg], np.abs(W[i * og:(i + 1) * og]), np.abs(b[i * og:(i + 1) * og]),
                                     a['stride'], a['pad']) for i in range(g)], axis=1)
    if strict:
        _exact(dst, bound, lim)
    if a['prelu'] is not None:
        slope = np.asarray(a['prelu'], np.float64)
        assert np.array_equal(slope, np.rint(slope)), 'PReLU slopes are integers here'
        bound = bound * np.maximum(1.0, np.abs(slope))[None, :, None, None]
        if mistake == 'prelu_shifted':
            slope = np.roll(slope, 1)
        y = np.where(y > 0, y, y * slope[None, :, None, None])
    elif a['relu']:
        y = np.maximum(y, 0.0)
    if a['pool']:
        y, bound = pool_ref(y), pool_ref(bound)
    if a['res'] is not None:
        r = ref[a['res']]
        off = a['res_ch_off'] + (4 if mistake == 'res_ch_off+4' else 0)
        r = r[:, (off + np.arange(cout)) % r.shape[1]]
        if a['res_up2']:
            iy, ix = np.arange(y.shape[2]) >> 1, np.arange(y.shape[3]) >> 1
            assert r.shape[2:] == ((y.shape[2] + 1) // 2, (y.shape[3] + 1) // 2)
            if mistake == 'up2_unshifted':
                iy, ix = np.minimum(np.arange(y.shape[2]), r.shape[2] - 1), np.minimum(np.arange(y.shape[3]), r.shape[3] - 1)
            r = r[:, :, iy][:, :, :, ix]
        assert r.shape == y.shape, (dst, r.shape, y.shape)
        y, bound = y + r, bound + np.abs(r)
    if strict:
        _exact(dst, bound, lim)
    if a['out2'] is not None:
        s2, h2 = (np.asarray(v, np.float64)[None, :, None, None] for v in (a['scale2'], a['shift2']))
        z = y * s2 + (0.0 if mistake == 'no_shift2' else h2)
        if strict:
            _exact(a['out2'], bound * np.abs(s2) + np.abs(h2), net.limit(a['out2']))
            assert np.array_equal(z, np.rint(z)), a['out2']
        off = a['out2_ch_off'] + (8 if mistake == 'out2_ch_off+8' else 0)
        full = ref[a['out2']].copy() if a['out2'] in ref else np.zeros((y.shape[0], chans[a['out2']]) + y.shape[2:])
        full[:, (off + np.arange(cout)) % full.shape[1]] = z
        ref[a['out2']] = full
    if a['out_ch_off'] or cout != chans[dst]:                       # into a slice: every other channel stays what its producer wrote
        full = ref[dst].copy() if dst in ref else np.zeros((y.shape[0], chans[dst]) + y.shape[2:])
        assert full.shape[2:] == y.shape[2:], (dst, full.shape, y.shape)
        full[:, a['out_ch_off']:a['out_ch_off'] + cout] = y
        y = full
    return y


def reference(net, fr, mistake=None):
    """float64 value of every named tensor of `net` for the uint8 RGB frames `fr`, as (N, C, H, W).  Asserts the exactness rule
    of the module text on every step.  A dw+pw block also yields '<dst>:mid', its depthwise intermediate.  `mistake`: see
    _conv_step (the rule is then not asserted: a wrong reference may break it)."""
    ref = {'input': input_ref(fr)}
    chans = {n: net.P.tensors[t][0] for n, t in net.tid.items()}
    for op, src, dst, a in net.steps:
        x = ref[src]
        lim = net.limit(dst)
        if op == 'conv':
            y = _conv_step(net, ref, x, dst, a, lim, chans, mistake)
        elif op == 'dwconv':
            y = dw_ref(x, a['W'], a['b'], a['stride'])
            _exact(dst, dw_ref(np.abs(x), np.abs(a['W']), np.abs(a['b']), a['stride']), lim)
            if a['relu']:
                y = np.maximum(y, 0.0)
        elif op == 'maxpool':
            y = pool_ref(x)
        elif op == 'copych':
            y = ref[dst].copy() if dst in ref else np.zeros((x.shape[0], chans[dst]) + x.shape[2:])
            assert y.shape[2:] == x.shape[2:]
            y[:, a['out_off']:a['out_off'] + a['ch']] = x[:, a['in_off']:a['in_off'] + a['ch']]
        elif op == 'dwpw':
            mid = np.maximum(dw_ref(x, a['Wd'], a['bd'], a['stride']), 0.0)
            _exact(dst + ':mid', dw_ref(np.abs(x), np.abs(a['Wd']), np.abs(a['bd']), a['stride']), LIMIT_SPLIT)
            y = np.maximum(conv_ref(mid, a['Wp'], a['bp']), 0.0)
            _exact(dst, conv_ref(mid, np.abs(a['Wp']), np.abs(a['bp'])), lim)
            ref[dst + ':mid'] = mid
        elif op == 'rfstem':                                        # float32 FMAs throughout, float32 out: 2^24
            (Ws, bs), rest = a['blocks'][0], a['blocks'][1:]
            y = np.maximum(conv_ref(x, Ws, bs, 2, 1), 0.0)
            _exact(dst + ':stem', conv_ref(x, np.abs(Ws), np.abs(bs), 2, 1), LIMIT_F32)
            for i, (Wd, bd, Wp, bp) in enumerate(rest):
                _exact(dst + ':dw%d' % i, dw_ref(y, np.abs(Wd), np.abs(bd), 1 + i), LIMIT_F32)
                y = np.maximum(dw_ref(y, Wd, bd, 1 + i), 0.0)
                _exact(dst + ':pw%d' % i, conv_ref(y, np.abs(Wp), np.abs(bp)), LIMIT_F32)
                y = np.maximum(conv_ref(y, Wp, bp), 0.0)
        else:
            raise AssertionError(op)
        if mistake is None:
            assert np.array_equal(y, np.rint(y)), dst               # integers: below the limit they have their bits
            _exact(dst, np.abs(y), lim)
        assert y.shape[1] == chans[dst], (dst, y.shape, chans[dst])
        ref[dst] = y
    return ref


# ---- the builders the tests share -----------------------------------------------------------------------------------------------
def selector(net, rng, name, C, *, k=1, wmax=64, halo=1, relu=False, f32=False, src='input', stride=1):
    """'input' -> conv k x k (3 -> C) -> `name`: integers, lo words and signs in use (see selector_weights)."""
    net.tensor(name, C, halo, f32=f32)
    W, b = selector_weights(rng, C, k, wmax if k == 1 else max(1, wmax // 8), density=1.0 if k == 1 else 0.5)
    net.conv(src, name, W, b, relu=relu, stride=stride)
    return name


def sink(net, rng, src, name, C, cout=64, variant=0):
    """`src` (halo 1) -> conv 3x3 pad 1 (C -> cout, one +-1 weight per tap and output) -> `name` (float32).  Its border outputs
    read the halo of `src`: exact only while that halo is still zero.  cout = 64 keeps a 32-channel-block `src` pre-split."""
    net.tensor(name, cout, 0, f32=True)
    W = np.zeros((cout, C, 3, 3))
    for o in range(cout):
        for t in range(9):
            W[o, rng.integers(0, C), t // 3, t % 3] = rng.choice([-1, 1])
    net.conv(src, name, W, np.zeros(cout), variant=variant)
    return name


DW_VARIANTS = ((1, 1), (1, 0), (2, 1), (2, 0))


def dwconv_net(precision, C, seed=1, variants=DW_VARIANTS):
    """C = 0: the depthwise convs read the 4-channel input tensor itself.  Else selector (3 -> C) -> 'src' -> one depthwise conv
    per (stride, ReLU) of `variants` -> 'dw_s<stride>_r<relu>'."""
    rng = np.random.default_rng(seed * 1000 + C)
    net = Net(precision)
    src, Cd = 'input', 4
    if C:
        src, Cd = selector(net, rng, 'src', C, wmax=6), C         # |src| <= 3 * 6 * 255 + 48: ten taps stay below 2^16
    for stride, relu in variants:
        W, b = dw_weights(rng, Cd, center=2 if C else 8)
        if not C:
            W[3] = 7.0                                               # the 4th input channel is 0: a tap that read a neighbour shows
        net.dwconv(src, net.tensor('dw_s%d_r%d' % (stride, relu), Cd), W, b, stride=stride, relu=bool(relu))
    return net


def maxpool_net(precision, C, in_halo, seed=2, with_sink=True):
    """C = 4: the pool reads the input tensor (halo `in_halo`).  Else selector 1x1 (bias and weights of both signs, no ReLU) ->
    'src' (halo `in_halo`) -> 2x2 max-pool -> 'pooled' (halo 1) -> sink conv 'after'."""
    rng = np.random.default_rng(seed * 1000 + C * 2 + in_halo)
    net = Net(precision, in_halo=in_halo if C == 4 else 0)
    src = 'input' if C == 4 else selector(net, rng, 'src', C, halo=in_halo, wmax=64)
    net.tensor('pooled', C, 1)
    net.maxpool(src, 'pooled')
    if with_sink:
        sink(net, rng, 'pooled', 'after', C, cout=64 if C % 32 == 0 else 32)
    if C != 4 and precision == 'f16x3':
        net.pin_exponent('src')
    return net


def copych_net(precision, c_src, c_dst, in_off, out_off, ch, dst_halo=1, src_halo=0, seed=3, with_sink=True):
    """selector A (3 -> c_dst, 3x3) -> 'dst' (every channel written first); selector B (3 -> c_src) -> 'src'; `ch` channels of
    'src' at `in_off` are copied to `out_off` of 'dst'; sink conv 'after' reads 'dst' with its halo."""
    rng = np.random.default_rng(seed * 1000 + c_src + c_dst + in_off + out_off)
    net = Net(precision)
    selector(net, rng, 'dst', c_dst, k=3, halo=dst_halo, wmax=64)
    selector(net, rng, 'src', c_src, halo=src_halo, wmax=64)
    net.copych('src', 'dst', in_off, out_off, ch)
    if with_sink:
        sink(net, rng, 'dst', 'after', c_dst, cout=64 if c_dst % 32 == 0 else 32)
    if precision == 'f16x3':
        net.pin_exponent('src')
    return net


def convpool_net(precision, seed=4):
    """selector (3 -> 32) -> 'src' -> conv 3x3 32 -> 64 + ReLU with the fused pool -> 'fused'; the same conv unfused -> 'full' ->
    2x2 max-pool -> 'pooled'."""
    rng = np.random.default_rng(seed)
    net = Net(precision)
    selector(net, rng, 'src', 32, wmax=6)
    W, b = sparse_weights(rng, (64, 32, 3, 3), 9, values=(-1, 1, 1), bias=100)
    net.tensor('fused', 64, 0, f32=True)
    net.conv('src', 'fused', W, b, relu=True, pool=True)
    net.tensor('full', 64, 0)
    net.conv('src', 'full', W, b, relu=True)
    net.tensor('pooled', 64, 0, f32=True)
    net.maxpool('full', 'pooled')
    return net


def dwpw_net(precision, C, cout, stride, seed=5):
    """selector (3 -> C) -> 'src' (float32: the block reads nothing else) -> [dw 3x3 + ReLU -> 1x1 + ReLU] -> 'block' (float32)."""
    rng = np.random.default_rng(seed * 100000 + C * 300 + cout + stride)
    net = Net(precision)
    selector(net, rng, 'src', C, wmax=2)
    Wd, bd = dw_weights(rng, C, center=1)
    Wp, bp = sparse_weights(rng, (cout, C, 1, 1), 4, values=(-2, -1, 1, 1, 2, 2))
    net.tensor('block', cout, 0, f32=True)
    net.dwpw('src', 'block', Wd, bd, Wp, bp, stride=stride)
    return net


def rfstem_net(precision, fused, seed=6):
    """The RetinaFace front as one op on the raw frames (no float input tensor exists) -> 'front': 16 channels at half resolution,
    or with `fused` the next block's 32 at a quarter.  Sparse +-1 weights, mostly +1 so that the ReLUs pass something on."""
    rng = np.random.default_rng(seed + int(fused))
    net = Net(precision, shape_only_input=True)
    vals = (-1, 1, 1, 1)
    blocks = [sparse_weights(rng, (8, 3, 3, 3), 5, vals), sparse_weights(rng, (8, 1, 3, 3), 4, vals) + sparse_weights(rng, (16, 8, 1, 1), 3, vals)]
    if fused:
        blocks.append(sparse_weights(rng, (16, 1, 3, 3), 4, vals) + sparse_weights(rng, (32, 16, 1, 1), 3, vals))
    net.tensor('front', 32 if fused else 16, 1, f32=True)
    net.rfstem('front', blocks)
    return net


def preprocess_net(kind, precision='f32'):
    """The smallest program of `kind`: its preprocess fills 'input' (halo 1), one 1x1 conv follows because a program needs an op."""
    rng = np.random.default_rng(7)
    net = Net(precision, kind=kind)
    net.tensor('out', 32, 0, f32=True)
    W, b = selector_weights(rng, 32, 1, 2)
    net.P.conv(net.tid['input'], net.tid['out'], W, b)             # not a step: only the RetinaFace input is integers
    return net


# ---- the conv output stage (tests/test_gpu_conv_exact.py) ------------------------------------------------------------------------
# Integer conventions on top of the rule of the module text: PReLU slopes are integers of {-2, -1, 0, 2, 3} per channel, the second
# output's scale is of {-2, -1, 1, 2} and its shift an integer, an input affine has scales of {-1, 1, 2} and integer shifts -- integer
# times integer stays an integer, and the bound is carried through the whole chain (bound * max(1, |slope|) + |shortcut|, then
# * |scale2| + |shift2|), each against the limit of the tensor it lands in.
def stage_weights(rng, cout, cin, k, nz=3, mags=(4, 1, 2, 1), bias=50, ranges=1):
    """(cout, cin, k, k): `nz` weights of +-mags[o % 4] per output channel o, the j-th of them in K range j % ranges (k_range_mask);
    integer bias.  The stepped magnitudes give the channels of the output different exponents in the half-float mode."""
    n = k * k * cin // 32
    W = np.zeros((cout, k * k * cin))
    for o in range(cout):
        for j in range(nz):
            r = j % ranges
            W[o, rng.integers(r * n // ranges * 32, (r + 1) * n // ranges * 32)] = rng.choice([-1, 1]) * mags[o % 4]
    return W.reshape(cout, k, k, cin).transpose(0, 3, 1, 2).copy(), rng.integers(-bias, bias + 1, cout).astype(np.float64)


EPILOGUES = {                                   # what the conv under test does behind its sums
    'plain': dict(),
    'relu_slices': dict(relu=True, out_slice=True, in_slice=True),     # reads channels 32.. of 'src', writes channels 32.. of 'out'
    'prelu': dict(prelu=True),
    'res32': dict(res=32),                                             # + shortcut channels 32..
    'res0_out2_slice': dict(res=0, out2=32),                           # + shortcut, second output into channels 32.. of 'out2'
    'prelu_res32_out2': dict(prelu=True, res=32, out2=0),
    'relu_out2': dict(relu=True, out2=0),
    'affine_prelu': dict(prelu=True, affine=True),                     # in_affine: nine border-class biases
    'affine_relu_res0': dict(relu=True, affine=True, res=0),
}
ALL_EPI = tuple(EPILOGUES)
NO_AFFINE = tuple(e for e in EPILOGUES if not e.startswith('affine'))

CONV_CASES = {                                  # C, cout, k, stride, groups, the epilogues run on it
    'c64_3x3': dict(C=64, cout=64, k=3, epi=ALL_EPI),
    'c128_3x3': dict(C=128, cout=128, k=3, epi=ALL_EPI),
    'c64to128_1x1_s2': dict(C=64, cout=128, k=1, stride=2, epi=('plain', 'res0_out2_slice', 'prelu_res32_out2')),
    'c256_3x3_g2': dict(C=256, cout=256, k=3, groups=2, epi=('relu_slices', 'prelu', 'res32', 'prelu_res32_out2')),
    # 40 channels at 132 of 192: no 8-channel boundary, so only the generic kernel's direct drain can run it
    'c128to40in192_1x1': dict(C=128, cout=40, k=1, out_total=192, out_off=132, epi=NO_AFFINE),
    'c192to128_7x7': dict(C=192, cout=128, k=7, epi=('plain', 'prelu_res32_out2')),
}
VARIANTS = ('generic', 'pipe64', 'split_2x2', 'split_1x4', 'split_2x4', 'split_2x2_w2', 'win_2x2')
SPLIT_VARIANTS = ('split_2x2', 'split_1x4', 'split_2x4', 'split_2x2_w2')
# (n, h, w) of the OUTPUT map: M = 1 (a single pixel), 45 (several images in one partial tile), 128 (exactly one tile), 132 (a full
# tile and a tail of 4), 270 (beyond 256, tiles crossing images)
SIZES = ((1, 1, 1), (3, 5, 3), (2, 8, 8), (1, 11, 12), (3, 9, 10))
THIN_SIZES = SIZES[1::2] + SIZES[4:]             # 45, 132, 270: what every case runs; the single pixel and the exact tile on two cases
FULL_SIZE_CASES = ('c128_3x3', 'c128to40in192_1x1')   # every kernel's staged and lean drains, and the direct drain
AFFINE_SIZE = (1, 6, 1)                        # one column: every pixel is of an 'only' class across and a first / middle / last down


def case_sizes(case, affine=False):
    return (SIZES if case in FULL_SIZE_CASES else THIN_SIZES) + ((AFFINE_SIZE,) if affine else ())


def win_patch_rows(h, w, k, BM):
    """csrc/conv_split.hip: ta_win_patch_rows for an h x w map read through a k x k window (halo k // 2)."""
    halo = k // 2
    wp, hp, n = w + 2 * halo, h + 2 * halo, BM - 1
    return n + -(-n // w) * (wp - w) + -(-n // (h * w)) * (hp - h) * wp + (k - 1) * wp + k


def variant_eligible(variant, precision, *, cout, k, stride=1, groups=1, staged=True, k_split=0, size=None, cin=64):
    """csrc/conv_igemm.hip: variant_eligible, for a conv whose input is float32 under 'generic' and in the precision's own format
    otherwise (cin % 32 == 0, so K is uniform)."""
    coutp = -(-cout // 32) * 32
    deep = k * k * cin // 32 >= 2
    if variant == 'generic':
        return groups == 1
    if not (deep and staged):
        return False
    if variant == 'pipe64':
        return coutp % 64 == 0 and groups == 1
    if variant in ('split_2x2', 'split_2x4'):
        return coutp % 128 == 0
    if variant == 'split_1x4':
        return coutp % 64 == 0 and (cout // groups) % 64 == 0
    if variant == 'split_2x2_w2':
        return coutp % 128 == 0 and k_split <= 1
    if variant == 'win_2x2':
        return (precision == 'f16x3' and stride == 1 and k_split <= 1 and k * k >= 4 and coutp % 128 == 0
                and (size is None or win_patch_rows(size[1], size[2], k, 128) <= 384))
    raise AssertionError(variant)


def conv_programs(case, variant, precision):
    """[(epilogue, io, sizes)] `variant` can run of CONV_CASES[case] in `precision`.  io 'f32': shortcut and outputs pinned to float32
    ('generic': the input as well); 'split': every tensor in the precision's pre-split format, where the split-role and window
    kernels take the lean drain for LEAN_EPILOGUES."""
    c = CONV_CASES[case]
    staged = c.get('out_off', 0) % 8 == 0
    out = []
    for epi in c['epi']:
        e = EPILOGUES[epi]
        sizes = [s for s in case_sizes(case, e.get('affine'))
                 if variant_eligible(variant, precision, cout=c['cout'], k=c['k'], stride=c.get('stride', 1), groups=c.get('groups', 1),
                                     staged=staged, size=s, cin=c['C'] // c.get('groups', 1))]
        for io in ('f32', 'split'):
            if io == 'split' and (precision == 'f32' or variant == 'generic'):
                continue
            if sizes:
                out.append((epi, io, tuple(sizes)))
    return out


KSPLIT_SIZES = ((3, 5, 3), (1, 11, 12), (3, 9, 10))


def frame_seed(size):
    return 1000 + size[0] * 977 + size[1] * 31 + size[2]


def frame_size(size, stride=1):
    """The frames whose conv output map is `size`."""
    n, h, w = size
    return (n, stride * (h - 1) + 1, stride * (w - 1) + 1)


def lean_expected(variant, precision, e, io, k_split=0):
    """Whether the launch runs conv_drain_fast (1) or the generic staged drain (0): a split-role or window kernel outside the f32
    mode, no K ranges, every tensor of the output stage pre-split, and epilogue `e` (a value of EPILOGUES) one of the shapes
    conv_drain_dispatch is compiled for -- plain / ReLU / PReLU, no activation + shortcut (+ second output), in_affine + PReLU."""
    plain = e.get('res') is None and e.get('out2') is None
    act = bool(e.get('relu') or e.get('prelu'))
    shape = (plain and bool(e.get('prelu'))) if e.get('affine') else (plain or (e.get('res') is not None and not act))
    return int((variant in SPLIT_VARIANTS or variant.startswith('win')) and precision != 'f32' and io == 'split' and k_split <= 1 and shape)


def _stage(net, rng, c, e, variant, io, *, stride=1, res_from=None, res_up2=0, k_split=0, nz=3, seed_affine=True):
    """'src' -> the conv under test with epilogue `e` -> 'out' (-> 'out2'), and a sink conv behind each output."""
    from terran_amd import lib
    C, cout, k, groups = c['C'], c['cout'], c['k'], c.get('groups', 1)
    pin = io == 'f32'
    in_off = 32 if e.get('in_slice') else 0
    selector(net, rng, 'src', C + in_off, halo=k // 2, wmax=1, f32=variant == 'generic')
    kw = dict(stride=stride, groups=groups, variant=lib.CONV_VARIANTS[variant], in_ch_off=in_off, k_split=k_split, relu=bool(e.get('relu')))
    if e.get('res') is not None:
        selector(net, rng, 'shortcut', cout + 32, k=3, halo=2, wmax=16, f32=pin, stride=2 if res_up2 else stride)
        kw.update(res='shortcut', res_ch_off=e['res'], res_up2=res_up2)
    out_total, out_off = c.get('out_total', cout + 64 if e.get('out_slice') else cout), c.get('out_off', 32 if e.get('out_slice') else 0)
    if out_total != cout:
        selector(net, rng, 'out', out_total, k=3, halo=1, wmax=16, f32=pin, stride=stride)      # every channel written before
    else:
        net.tensor('out', cout, 1, f32=pin)
    if e.get('out2') is not None:
        if e['out2']:
            selector(net, rng, 'out2', cout + 32, k=3, halo=1, wmax=16, f32=pin, stride=stride)
        else:
            net.tensor('out2', cout, 1, f32=pin)
        kw.update(out2='out2', out2_ch_off=e['out2'], scale2=rng.choice([-2, -1, 1, 2], cout).astype(np.float64),
                  shift2=rng.integers(-100, 101, cout).astype(np.float64))
    if e.get('prelu'):
        kw['prelu'] = rng.choice([-2, -1, 0, 2, 3], cout).astype(np.float64)
    if e.get('affine'):
        kw['in_affine'] = (rng.choice([-1, 1, 2], C).astype(np.float64), rng.integers(-8, 9, C).astype(np.float64))
    W, b = stage_weights(rng, cout, C // groups, k, nz=nz, ranges=max(k_split, 1))
    net.conv('src', 'out', W, b, out_ch_off=out_off, **kw)
    # the sinks are pinned as well, to another kernel than the one under test: the launch counts then say which conv ran where
    # (40 or 72 channels are no whole K slabs: those sinks are the generic kernel's, as the conv under test is)
    net.sink_variant = sv = 'pipe64' if variant != 'pipe64' and cout % 32 == 0 else ('generic' if pin else 'split_1x4')
    sink(net, rng, 'out', 'after', out_total, variant=lib.CONV_VARIANTS[sv])
    if e.get('out2') is not None:
        sink(net, rng, 'out2', 'after2', cout + e['out2'], variant=lib.CONV_VARIANTS[sv])
    n_sel = sum(1 for s in net.steps if s[1] == 'input')
    net.counts = {variant: 1}                                       # what Context.conv_counts() must show after one forward
    for v, n in (('generic', n_sel), (sv, 2 if e.get('out2') is not None else 1)):
        net.counts[v] = net.counts.get(v, 0) + n
    if lean_expected(variant, net.precision, e, io, k_split):
        net.counts['lean_epilogue'] = 1
    net.names = [n for n in ('src', 'shortcut', 'out', 'out2', 'after', 'after2') if n in net.tid]
    return net


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def epilogue_net(precision, case, variant, epi, io='f32'):
    """selector (3 -> C) -> 'src'; a 3x3 selector -> 'shortcut' (32 channels wider than cout, halo 2); the conv of CONV_CASES[case]
    with EPILOGUES[epi], pinned to `variant` -> 'out' (halo 1; a slice of a tensor a 3x3 selector has written where the epilogue or
    the case says so) and 'out2'; sink convs 'after' / 'after2' read both with their halos.  The weights depend on (case, epi) alone:
    every variant, io and precision of a case computes the same numbers."""
    c = CONV_CASES[case]
    return _stage(Net(precision), np.random.default_rng(_seed('epilogue', case, epi)), c, EPILOGUES[epi], variant, io, stride=c.get('stride', 1))


UP2_CASES = ('c64_3x3', 'c128_3x3')
UP2_EPILOGUES = {'relu_res0': dict(relu=True, res=0), 'res32': dict(res=32), 'res32_out2': dict(res=32, out2=0)}


def up2_net(precision, case, variant, epi, io='f32'):
    """As epilogue_net, but 'shortcut' comes from a STRIDE-2 3x3 selector on the same frames -- ceil(h / 2) x ceil(w / 2) -- and the
    conv under test reads it at (y >> 1, x >> 1) (RetinaFace's FPN merge, pack/retinaface.py)."""
    return _stage(Net(precision), np.random.default_rng(_seed('up2', case, epi)), CONV_CASES[case], UP2_EPILOGUES[epi], variant, io, res_up2=1)


def up2_programs(case, variant, precision):
    c = CONV_CASES[case]
    out = []
    for epi in UP2_EPILOGUES:
        sizes = tuple(s for s in case_sizes(case) if variant_eligible(variant, precision, cout=c['cout'], k=c['k'], size=s, cin=c['C']))
        out += [(epi, io, sizes) for io in ('f32', 'split') if sizes and not (io == 'split' and (precision == 'f32' or variant == 'generic'))]
    return out


KSPLIT_CASES = {'c256_3x3': dict(C=256, cout=128, k=3), 'c512_1x1': dict(C=512, cout=128, k=1)}
KSPLIT_EPILOGUES = {'relu': dict(relu=True), 'prelu': dict(prelu=True), 'res32': dict(res=32), 'res0_out2_slice': dict(res=0, out2=32),
                    'affine_prelu': dict(prelu=True, affine=True)}                  # in_affine: 3x3 only, no second output (Program.conv)
KSPLIT_VARIANTS = ('split_2x2', 'split_2x4', 'split_1x4')                            # the 3-stage split-role kernels know K ranges
KSPLITS = (2, 4)


def ksplit_net(precision, case, variant, epi, k_split, io='f32'):
    """As epilogue_net with K cut in `k_split` ranges: the kernels write raw partial sums, splitk_reduce_kernel runs the whole epilogue.
    Every output channel has a weight in every range."""
    return _stage(Net(precision), np.random.default_rng(_seed('ksplit', case, epi, k_split)), KSPLIT_CASES[case], KSPLIT_EPILOGUES[epi],
                  variant, io, k_split=k_split, nz=4)


def ksplit_programs(case, precision):
    """[(epilogue, k_split, io)] of KSPLIT_CASES[case]."""
    k = KSPLIT_CASES[case]['k']
    return [(epi, ks, io) for epi, e in KSPLIT_EPILOGUES.items() if k == 3 or not e.get('affine') for ks in KSPLITS
            for io in (('f32',) if precision == 'f32' else ('f32', 'split'))]


# ---- the cases of tests/test_gpu_layers_exact.py (tests/test_exact_programs_cpu.py walks the same lists) ---------------------------
PRECISIONS = ('f32', 'f16x3', 'bf16x3')
DW_CHANNELS = (0, 4, 32, 64)                                         # 0: straight on the input tensor
DW_SHAPES = ((1, 1), (1, 6), (7, 1), (2, 2), (9, 11), (10, 12))
POOL_CHANNELS = (4, 32, 64, 96)
POOL_SHAPES = ((2, 2), (3, 3), (2, 9), (9, 2), (7, 10), (11, 13))
COPY_CASES = {                                                       # (c_src, c_dst, in_off, out_off, ch, dst_halo, src_halo)
    '64of96_into128_at32': (96, 128, 32, 32, 64, 1, 0),
    '32of64_first_into96_last': (64, 96, 0, 64, 32, 1, 2),
    'whole32_into64_at0': (32, 64, 0, 0, 32, 1, 1),
    'offset4_falls_back_to_f32': (64, 96, 4, 36, 32, 1, 0),
}
COPY_SHAPES = ((1, 1), (5, 7), (9, 16))
CONVPOOL_SHAPES = ((2, 2), (5, 7), (8, 8), (9, 16))
DWPW_CASES = ((64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (32, 32, 1), (32, 64, 2), (96, 40, 1), (64, 24, 1))
DWPW_SHAPES = ((5, 7), (9, 16))
RFSTEM_SHAPES = ((1, 27, 123), (1, 29, 125), (2, 57, 249), (1, 5, 7), (1, 56, 248), (1, 31, 126), (3, 16, 16))

# One case per grid-stride kernel whose work items (the `total` of its ta_launch_*) just exceed the 2048 x 256 threads a launch is
# capped at, so that the loop's second trip runs: (frame h, w) and the total, for one image, float32.
GRID_CAP = 2048 * 256
SECOND_TRIP = {
    'preprocess': ((725, 724), 725 * 724),                          # n h w pixels
    'dwconv': ((257, 256), 257 * 256 * (32 // 4)),                  # n ho wo (C / 4), stride 1, C = 32
    'maxpool': ((364, 362), 182 * 181 * (64 // 4)),                 # n ho wo (C / 4) of the POOLED map, C = 64
    'copych': ((257, 256), 257 * 256 * (32 // 4)),                  # n h w (ch / 4), 32 channels copied
}
