"""Small op programs whose right answer is ONE bit pattern, and their float64 reference (no GPU import).

The HBM-bound layer kernels (csrc/layers.hip: preprocess, depthwise 3x3, 2x2 max-pool, channel-slice copy, the RetinaFace
front) and the format helpers they go through (csrc/act_format.h: ta_ld4 / ta_st4 / ta_ld1) move and combine numbers; on
inputs whose values and partial sums are exactly representable in every storage format there is nothing to round, so a
tolerance has nothing to forgive: any mistake in addressing, format or exponent changes the bits.

The rule (`reference` asserts it, DESIGN.md states it): every value a program holds and every partial sum of the products
that make it is an integer of at most 16 significant bits -- what a bf16 hi + lo pair carries (the half-float pair carries
22) -- and at most 65504, the end of the half-float range for the tensors the packer stores unscaled.  A tensor that is
only ever held as float32 (pinned f32 and read by no op, or inside the all-float32 front kernel) may reach 2^24.  The
bound is taken over sum |w| |x| + |b|, so it holds for every summation order a kernel may choose.

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
        t0 = P.tensor(4, in_halo, alias_of=-2 if shape_only_input else -1, name='input')
        self.tid['input'] = t0
        P.input_tensor = t0
        P.input_stats = PIXEL_STATS

    def tensor(self, name, c, halo=0, f32=False):
        self.tid[name] = self.P.tensor(c, halo, name=name, f32=f32)
        return name

    def conv(self, src, dst, W, b, *, stride=1, pad=None, relu=False, pool=False):
        self.P.conv(self.tid[src], self.tid[dst], W, b, stride=stride, pad=pad, act=pack.ACT_RELU if relu else pack.ACT_NONE, pool=pool)
        self.steps.append(('conv', src, dst, dict(W=W, b=b, stride=stride, pad=W.shape[2] // 2 if pad is None else pad, relu=relu, pool=pool)))

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


def reference(net, fr):
    """float64 value of every named tensor of `net` for the uint8 RGB frames `fr`, as (N, C, H, W).  Asserts the exactness rule
    of the module text on every step.  A dw+pw block also yields '<dst>:mid', its depthwise intermediate."""
    ref = {'input': input_ref(fr)}
    chans = {n: net.P.tensors[t][0] for n, t in net.tid.items()}
    for op, src, dst, a in net.steps:
        x = ref[src]
        lim = net.limit(dst)
        if op == 'conv':
            y = conv_ref(x, a['W'], a['b'], a['stride'], a['pad'])
            _exact(dst, conv_ref(np.abs(x), np.abs(a['W']), np.abs(a['b']), a['stride'], a['pad']), lim)
            if a['relu']:
                y = np.maximum(y, 0.0)
            if a['pool']:
                y = pool_ref(y)
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
        assert np.array_equal(y, np.rint(y)), dst                   # integers: below the limit they have their bits
        _exact(dst, np.abs(y), lim)
        assert y.shape[1] == chans[dst], (dst, y.shape, chans[dst])
        ref[dst] = y
    return ref


# ---- the builders the tests share -----------------------------------------------------------------------------------------------
def selector(net, rng, name, C, *, k=1, wmax=64, halo=1, relu=False, f32=False, src='input'):
    """'input' -> conv k x k (3 -> C) -> `name`: integers, lo words and signs in use (see selector_weights)."""
    net.tensor(name, C, halo, f32=f32)
    W, b = selector_weights(rng, C, k, wmax if k == 1 else max(1, wmax // 8), density=1.0 if k == 1 else 0.5)
    net.conv(src, name, W, b, relu=relu)
    return name


def sink(net, rng, src, name, C, cout=64):
    """`src` (halo 1) -> conv 3x3 pad 1 (C -> cout, one +-1 weight per tap and output) -> `name` (float32).  Its border outputs
    read the halo of `src`: exact only while that halo is still zero.  cout = 64 keeps a 32-channel-block `src` pre-split."""
    net.tensor(name, cout, 0, f32=True)
    W = np.zeros((cout, C, 3, 3))
    for o in range(cout):
        for t in range(9):
            W[o, rng.integers(0, C), t // 3, t % 3] = rng.choice([-1, 1])
    net.conv(src, name, W, np.zeros(cout))
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
