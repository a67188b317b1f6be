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

The tolerance modes (TOLERANCE_MODES: 'f16', 'f16x2', 'bf16') drop words on purpose, so their rule is per mode and per storage
format, and `reference` asserts it per tensor from the packed program's tensor_formats(), scales and weight-row exponents (class
Rounding: each limit is the format's own rounding function, and a value obeys the rule when that function leaves it unchanged):
- a TA_FMT_F16 tensor holds one IEEE half per value: 11 significant bits (10 stored + the implicit one) at the channel's exponent,
  |x 2^a| <= 65504; TA_FMT_SPLIT16 holds hi + lo halves: 22 bits in the same range; TA_FMT_SPLIT two bf16 words: 16 bits; float32: 24;
- 'f16' reads 11 bits of either operand (the hi half of a weight row, a TA_FMT_F16 tensor as it is, a float32 one rounded in registers);
- 'f16x2' computes (w_hi + w_lo) * x_hi: the activations a conv reads have 11 bits (x_lo = 0), the weights may use the whole pair;
- 'bf16' computes hi * hi on bf16 words: 8 significant bits per operand;
- every partial sum (sum |w| |x| + |b|) stays below 2^24, the float32 accumulator's integers.
Programs of family 'exact' obey all of this, so no rounding changes a value and the reference equals plain float64 arithmetic.
Programs of family 'rounded' break a bit count on purpose; `reference` then applies the one rounding the mode defines -- to nearest
even when an operand is formed or a tensor is stored -- in float64, exactly (products and sums still stay exact below 2^24).
The sink convs of an 'f16x2' / 'bf16' program run in the sister mode that reads both words ('f16x3' / 'bf16x3'), so what the conv under
test stores may use its whole format; 'f16' has no such sister for a TA_FMT_F16 tensor, whose 11 bits every reader gets anyway.

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



# ---- the roundings of the tolerance modes, in float64 ---------------------------------------------------------------------------
TOLERANCE_MODES = ('f16', 'f16x2', 'bf16')
SISTER_MODE = {'f16': 'f16', 'f16x2': 'f16x3', 'bf16': 'bf16x3'}     # reads both words of what the mode stores
HALF = dict(bits=11, emin=-24, top=F16_MAX)      # IEEE half: 10 stored bits + the implicit one, subnormal quantum 2^-24, ends at 65504
BF16 = dict(bits=8, emin=-133, top=np.inf)       # bfloat16: 7 stored bits + the implicit one, float32's exponents


def rne(v, bits, emin, top, toward_zero=False):
    """float64 `v` rounded to `bits` significant bits, to nearest even (or toward zero), quantum never below 2^emin."""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(v)                                             # |v| in [2^(e - 1), 2^e)
    q = np.maximum(e - bits, emin)
    t = np.ldexp(v, -q)
    r = np.ldexp(np.trunc(t) if toward_zero else np.rint(t), q)    # np.rint: halves to even
    assert not r.size or np.abs(r).max() <= top, 'a value leaves the range of its format (%g)' % np.abs(r).max()
    return r


def pair(v, word):
    """hi + lo of two `word`-format words: hi = rne(v), lo = rne(v - hi)."""
    hi = rne(v, **word)
    return hi + rne(v - hi, **word)


class Rounding:
    """What a packed tolerance-mode program rounds where.  Everything is per channel in STORED units (value times 2^a[c], the
    packer's exponents) and comes back in real units.  `changed` collects (tensor or op, what) wherever a rounding was not the identity."""

    def __init__(self, net, mistake=None):
        from terran_amd.pack import FMT_F16, FMT_F32, FMT_SPLIT, FMT_SPLIT16
        P = net.P
        P.blob()                                                   # settles formats, exponents and the weight-row exponents
        self.net, self.mistake, self.changed = net, mistake, set()
        self.half = dict(HALF, top=np.inf) if mistake else HALF        # (a wrong reference may leave the range)
        self.fmt = {n: P.tensor_formats()[t] for n, t in net.tid.items()}
        self.a = {n: P.scales[t].astype(np.int32) for n, t in net.tid.items()}
        self.F16, self.F32, self.SPLIT, self.SPLIT16 = FMT_F16, FMT_F32, FMT_SPLIT, FMT_SPLIT16

    def _note(self, got, want, key):
        if not np.array_equal(got, want):
            self.changed.add(key)
        return got

    def store(self, name, y, ch_off=0):
        """y (N, c, H, W) real values written into channels ch_off.. of tensor `name` -> what a reader of every word gets back."""
        a = self.a[name][ch_off:ch_off + y.shape[1]][None, :, None, None]
        s, f = np.ldexp(y, a), self.fmt[name]
        if f == self.F16:
            r = rne(s, toward_zero=self.mistake == 'store_truncated', **self.half)
        elif f == self.SPLIT16:
            r = pair(s, self.half)
        elif f == self.SPLIT:
            r = pair(s, BF16)
        else:
            r = s.astype(np.float32).astype(np.float64)
        # the range guard of a program with half-float convs watches every store, float32 ones included (conv_common.h: ta_range_report)
        assert self.mistake or self.net.precision == 'bf16' or not r.size or np.abs(r).max() <= F16_MAX, '%s: %g leaves the half-float range' % (name, np.abs(r).max())
        return self._note(np.ldexp(r, -a), y, (name, 'store'))

    def read(self, name, x, mode):
        """The activation operand a conv of arithmetic mode `mode` forms from tensor `name` (x: all its channels, real values)."""
        a = self.a[name][None, :, None, None]
        s = np.ldexp(x, a)
        if mode in ('f16', 'f16x2') and not (mode == 'f16x2' and self.mistake == 'x_lo_kept'):
            s = rne(s, **self.half)            # the hi half of a pair, a TA_FMT_F16 value itself, or a float32 one rounded in registers
        elif mode == 'bf16':
            s = rne(s, **BF16)
        return self._note(np.ldexp(s, -a), x, (name, 'read by ' + mode))

    def weights(self, a_step, W, src):
        """The weight operand of the conv of step dict `a_step`: W (cout, cin_g, kh, kw) real -> what the mode multiplies with, real.
        Rows are packed times 2^(wexp[co] - a_in[c]) (pack/layout.py: split_f16_rows, split_bf16_rows; program.py: rows64)."""
        mode, g = a_step['precision'], a_step['groups']
        cout, cin = W.shape[:2]
        wexp = np.asarray(self.net.P._fold[a_step['op']]['wexp'][:cout], np.int32)
        a_in = self.a[src][a_step['in_ch_off']:a_step['in_ch_off'] + cin * g].reshape(g, cin)
        e = wexp[:, None] - np.repeat(a_in, cout // g, axis=0)                       # (cout, cin)
        s = np.ldexp(W, e[:, :, None, None])
        word = self.half if mode in ('f16', 'f16x2', 'f16x3') else BF16
        if mode in ('f16', 'bf16') or (mode == 'f16x2' and self.mistake == 'w_lo_dropped'):
            r = rne(s, **word)
        elif mode == 'f32':
            r = s
        else:
            r = pair(s, word)
        return self._note(np.ldexp(r, -e[:, :, None, None]), W, (a_step['op'], 'weights'))


# ---- programs -------------------------------------------------------------------------------------------------------------------
class Net:
    """A pack.Program plus the recipe `reference` replays in float64.  Tensors are addressed by name."""

    def __init__(self, precision, kind=pack.MODEL_RETINAFACE, in_halo=1, shape_only_input=False, pixel_shift=0, family='exact'):
        self.P = P = pack.Program(kind, precision)
        self.precision = precision
        self.pixel_shift = pixel_shift                            # the frames are `frames(...) >> pixel_shift`: 0 .. 255 >> shift
        self.quantum = LO_QUANTUM if precision == 'f16x2' else 0      # every value is an integer times 2^quantum
        self.family = family                                      # 'exact': no rounding changes a value; 'rounded': one does (module text)
        self.tid = {}
        self.steps = []
        self.mid_ops = {}                                         # dst name -> op index of a dw+pw block
        self.conv_ops = {}                                        # dst name -> op index of the last conv that writes it
        t0 = P.tensor(4, in_halo, alias_of=-2 if shape_only_input else -1, name='input')
        self.tid['input'] = t0
        P.input_tensor = t0
        top = 256 >> pixel_shift                                  # moments of uniform 0 .. top - 1
        P.input_stats = (np.array([(top - 1) / 2.0] * 3 + [0.0]), np.array([(top * top - 1.0) / 12.0] * 3 + [0.0]))

    def tensor(self, name, c, halo=0, f32=False):
        self.tid[name] = self.P.tensor(c, halo, name=name, f32=f32)
        return name

    def conv(self, src, dst, W, b, *, stride=1, pad=None, relu=False, pool=False, prelu=None, res=None, res_ch_off=0, res_up2=0,
             out2=None, out2_ch_off=0, scale2=None, shift2=None, out_ch_off=0, in_ch_off=0, cin_p=None, groups=1, k_split=0,
             in_affine=None, variant=0, precision=None):
        """pack.Program.conv with tensors by name (`precision`: this op alone runs in another arithmetic mode).
        The output stage in the kernels' order: conv + bias (in_affine: of scale * x +
        shift, zero-padded AFTER the affine), ReLU / PReLU, + res[:, res_ch_off:+cout, y >> res_up2, x >> res_up2], store into the
        slice at out_ch_off, then out2[:, out2_ch_off:+cout] = out * scale2 + shift2."""
        act = pack.ACT_PRELU if prelu is not None else (pack.ACT_RELU if relu else pack.ACT_NONE)
        tid = lambda n: -1 if n is None else self.tid[n]
        self.conv_ops[dst] = oi = len(self.P.ops)
        self.P.conv(self.tid[src], self.tid[dst], W, b, stride=stride, pad=pad, act=act, pool=pool, prelu=prelu, res=tid(res),
                    res_ch_off=res_ch_off, res_up2=res_up2, out2=tid(out2), out2_ch_off=out2_ch_off, scale2=scale2, shift2=shift2,
                    out_ch_off=out_ch_off, in_ch_off=in_ch_off, cin_p=cin_p, groups=groups, k_split=k_split, in_affine=in_affine,
                    variant=variant, precision=precision)
        self.steps.append(('conv', src, dst, dict(op=oi, src=src, precision=precision or self.precision, W=W, b=b, stride=stride, pad=W.shape[2] // 2 if pad is None else pad, relu=relu, pool=pool,
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


MODE_MISTAKES = ('x_lo_kept', 'w_lo_dropped', 'store_truncated', 'slab64_second_half_swapped')     # of the tolerance modes
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


def _conv_step(net, ref, x, dst, a, lim, chans, mistake, R=None):
    """One conv of `reference` with its whole output stage.  Returns what `dst` holds afterwards; writes `out2` into ref itself.
    `mistake`: one of MISTAKES (the deliberately wrong references of tests/test_exact_programs_cpu.py), or 'fold': in_affine by the
    packer's folded weights and border-class biases instead of by its meaning."""
    strict = mistake is None
    W, b, g = np.asarray(a['W'], np.float64), np.asarray(a['b'], np.float64), a['groups']
    cout, cin = W.shape[:2]
    lim2 = net.limit(a['out2']) if a['out2'] is not None and R is None else np.ldexp(LIMIT_F32, net.quantum)
    wq = (lambda w: R.weights(a, w, a['src'])) if R else (lambda w: w)     # a tolerance mode: the operands as the mode forms them
    if R:
        x = R.read(a['src'], x, a['precision'])
        if mistake == 'slab64_second_half_swapped' and dst == 'out' and R.fmt[a['src']] == R.F16:
            W = W.copy()                                                    # tap (0, 0): the 32-channel halves of every 64-channel slab
            W[:, :, 0, 0] = W[:, :, 0, 0].reshape(cout, cin // 64, 2, 32)[:, :, ::-1].reshape(cout, cin)
    xin = x[:, a['in_ch_off']:a['in_ch_off'] + cin * g]
    assert xin.shape[1] == cin * g
    xabs = np.abs(xin)
    if a['k_split'] > 1 and mistake == 'k_range_dropped':
        W = W * ~k_range_mask(W, a['k_split'], 1)
    aff = a['in_affine']
    if aff is not None and (mistake in ('fold', 'corner_as_edge') or R):      # (a tolerance mode rounds the FOLDED weights)
        Wf, b16 = pack.fold_input_affine(W, b, *aff)
        if strict:
            sc, sh = (np.asarray(v, np.float64)[None, :, None, None] for v in aff)
            _exact(dst, conv_ref(xabs * np.abs(sc) + np.abs(sh), np.abs(W), np.abs(b), 1, 1), lim)
        y = conv_ref(xin, wq(Wf), np.zeros(cout), 1, 1)
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
        cg, og, Wq = cin, cout // g, wq(W)
        y = np.concatenate([conv_ref(xin[:, i * cg:(i + 1) * cg], Wq[i * og:(i + 1) * og], b[i * og:(i + 1) * og], a['stride'], a['pad'])
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
            _exact(a['out2'], bound * np.abs(s2) + np.abs(h2), lim2)
            assert np.array_equal(np.ldexp(z, -net.quantum), np.rint(np.ldexp(z, -net.quantum))), a['out2']
        if R:
            z = R.store(a['out2'], z, a['out2_ch_off'])
        off = a['out2_ch_off'] + (8 if mistake == 'out2_ch_off+8' else 0)
        full = ref[a['out2']].copy() if a['out2'] in ref else np.zeros((y.shape[0], chans[a['out2']]) + y.shape[2:])
        full[:, (off + np.arange(cout)) % full.shape[1]] = z
        ref[a['out2']] = full
    if R:
        y = R.store(dst, y, a['out_ch_off'])
    if a['out_ch_off'] or cout != chans[dst]:                       # into a slice: every other channel stays what its producer wrote
        full = ref[dst].copy() if dst in ref else np.zeros((y.shape[0], chans[dst]) + y.shape[2:])
        assert full.shape[2:] == y.shape[2:], (dst, full.shape, y.shape)
        full[:, a['out_ch_off']:a['out_ch_off'] + cout] = y
        y = full
    return y


def reference(net, fr, mistake=None):
    """float64 value of every named tensor of `net` for the uint8 RGB frames `fr`, as (N, C, H, W).  Asserts the exactness rule
    of the module text on every step.  A dw+pw block also yields '<dst>:mid', its depthwise intermediate.  `mistake`: see
    _conv_step (the rule is then not asserted: a wrong reference may break it).  A program of a tolerance mode is packed here (its
    exponents decide where a half float rounds); net.rounding.changed then says which roundings were not the identity."""
    ref = {'input': input_ref(fr)}
    assert fr.max() < 256 >> net.pixel_shift, 'the frames of this program are frames(...) >> %d' % net.pixel_shift
    chans = {n: net.P.tensors[t][0] for n, t in net.tid.items()}
    R = net.rounding = Rounding(net, mistake) if net.precision in TOLERANCE_MODES else None
    for op, src, dst, a in net.steps:
        x = ref[src]
        lim = net.limit(dst) if R is None else np.ldexp(LIMIT_F32, net.quantum)      # 2^24 quanta: the float32 accumulator's integers
        if op == 'conv':
            y = _conv_step(net, ref, x, dst, a, lim, chans, mistake, R)
            if R and mistake is None and net.family == 'exact':
                assert not R.changed, "%s: the exactness rule of mode '%s' does not hold: %s" % (dst, net.precision, sorted(map(str, R.changed)))
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
            yq = np.ldexp(y, -net.quantum)
            assert np.array_equal(yq, np.rint(yq)), dst               # integers (of the net's quantum): below the limit they have their bits
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


def sink(net, rng, src, name, C, cout=64, variant=0, precision=None, taps=range(9)):
    """`src` (halo 1) -> conv 3x3 pad 1 (C -> cout, one +-1 weight per tap and output) -> `name` (float32).  Its border outputs
    read the halo of `src`: exact only while that halo is still zero.  cout = 64 keeps a 32-channel-block `src` pre-split."""
    net.tensor(name, cout, 0, f32=True)
    W = np.zeros((cout, C, 3, 3))
    for o in range(cout):
        for t in taps:                                              # (fewer taps: a sink whose sums must stay small)
            W[o, rng.integers(0, C), t // 3, t % 3] = rng.choice([-1, 1])
    net.conv(src, name, W, np.zeros(cout), variant=variant, precision=precision)
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


def cover_inputs(rng, W, values):
    """1x1 weights W (cout, C, 1, 1), in place: every input channel that no output row drew gets ONE weight of `values`, the idle
    channels dealt round the rows in a random order (at most ceil(idle / cout) more per row).  What was drawn before stays."""
    cout = W.shape[0]
    idle = np.flatnonzero(~W[:, :, 0, 0].any(axis=0))
    rows = rng.permutation(cout)
    for i, c in enumerate(idle):
        W[rows[i % cout], c, 0, 0] = rng.choice(values)
    return W


def dwpw_net(precision, C, cout, stride, seed=5):
    """selector (3 -> C) -> 'src' (float32: the block reads nothing else) -> [dw 3x3 + ReLU -> 1x1 + ReLU] -> 'block' (float32).
    Each output row draws 4 weights of +-1, +-2; the input channels left without one then get one (cover_inputs), a row without a
    positive weight gets one, and the depthwise taps of an all-negative 'src' channel are negative: a channel that reaches no output,
    through a zero weight or a ReLU that cuts it everywhere, cannot show a wrong tap, bias or slab (the CPU tests perturb them).  |src| <= 3 * 2 * 255 + 16 = 1546, |mid| <= 9 * 1546 + 50 < 2^14, and a row of
    C = 1024 into 64 outputs has about 16 weights: 16 * 2 * 13964 + 20 < 2^19, far below the 2^24 of the float32-only 'block'."""
    rng = np.random.default_rng(seed * 100000 + C * 300 + cout + stride)
    net = Net(precision)
    net.tensor('src', C, 1)
    Ws, bs = selector_weights(rng, C, 1, 2)        # (selector(): the same draw)
    idle = np.flatnonzero(~Ws.any(axis=(1, 2, 3)))   # a channel of three zero weights is one constant: no tap of it could be told from another
    Ws[idle, idle % 3, 0, 0] = np.where(idle % 8 == 5, -1.0, 1.0)
    net.conv('input', 'src', Ws, bs)
    Wd, bd = dw_weights(rng, C, center=1)
    values = (-2, -1, 1, 1, 2, 2)
    Wp, bp = sparse_weights(rng, (cout, C, 1, 1), 4, values=values)
    cover_inputs(rng, Wp, values)
    # Signs, not magnitudes: half the channels of 'src' have one sign throughout (selector weights of one sign), and taps or a row that
    # lean against the mean of what they read are 0 behind their ReLU at EVERY pixel.  Turn those round, by the means of uniform pixels.
    sel = net.steps[-1][3]
    src_mean = 127.5 * sel['W'].sum(axis=(1, 2, 3)) + sel['b']
    Wd[Wd.sum(axis=(1, 2, 3)) * src_mean < 0] *= -1
    mid_mean = np.maximum(Wd.sum(axis=(1, 2, 3)) * src_mean + bd, 0.0)
    Wp[Wp[:, :, 0, 0] @ mid_mean + bp < 0] *= -1
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


def case_sizes(case, affine=False, precision='f32'):
    full = MODE_FULL_SIZE_CASES if precision in ('f16', 'f16x2', 'bf16') else FULL_SIZE_CASES
    return (SIZES if case in full else THIN_SIZES) + ((AFFINE_SIZE,) if affine else ())


def win_patch_rows(h, w, k, BM):
    """csrc/conv_split.hip: ta_win_patch_rows for an h x w map read through a k x k window (halo k // 2)."""
    halo = k // 2
    wp, hp, n = w + 2 * halo, h + 2 * halo, BM - 1
    return n + -(-n // w) * (wp - w) + -(-n // (h * w)) * (hp - h) * wp + (k - 1) * wp + k


def variant_eligible(variant, precision, *, cout, k, stride=1, groups=1, staged=True, k_split=0, size=None, cin=64):
    """csrc/conv_igemm.hip: variant_eligible, for a conv whose input is float32 where src_is_f32 says so and in the precision's own
    format otherwise (cin % 32 == 0, so K is uniform).  'f16': one 64-channel slab already counts as deep, pipe64 reads float32 only
    (src_is_f32), and a TA_FMT_F16 input takes no groups (pack/storage.py), so no split-role kernel runs a grouped conv."""
    coutp = -(-cout // 32) * 32
    deep = k * k * cin // 32 >= 2 or precision == 'f16'
    if variant == 'generic':
        return groups == 1
    if not (deep and staged):
        return False
    if variant == 'pipe64':
        return coutp % 64 == 0 and groups == 1
    if precision == 'f16' and (groups > 1 or cin % 64):
        return False
    if variant in ('split_2x2', 'split_2x4'):
        return coutp % 128 == 0
    if variant == 'split_1x4':
        return coutp % 64 == 0 and (cout // groups) % 64 == 0
    if variant == 'split_2x2_w2':
        return coutp % 128 == 0 and k_split <= 1
    if variant == 'win_2x2':
        return (precision in ('f16x3', 'f16x2') and stride == 1 and k_split <= 1 and k * k >= 4 and coutp % 128 == 0
                and (size is None or win_patch_rows(size[1], size[2], k, 128) <= 384))
    raise AssertionError(variant)


def src_is_f32(variant, precision):
    """The conv under test reads a float32 'src': the generic kernel always, pipe64 in the 'f16' mode."""
    return variant == 'generic' or (variant == 'pipe64' and precision == 'f16')


MODE_PIXEL_SHIFT = {'f16': 5, 'f16x2': 5, 'bf16': 2}
# The frames of an 'exact' program of a tolerance mode are frames(...) >> shift, so that the bit counts of the module text hold:
#   'f16'   0 .. 7:  |src| <= 3 * 7 + 8 = 29, |sums| <= 4 * 4 * 29 + 50 = 514, times a PReLU slope of 3 and plus a shortcut of at most
#           27 * 7 + 8 = 197: 1739, and the second output (2 y + 100) / 2 <= 1789 -- all below 2^11, what a TA_FMT_F16 tensor holds;
#   'f16x2' 0 .. 7 as well (x_lo = 0); one weight per output channel is 1 + 2^-11 times its magnitude (hi 1, lo 2^-11), so the values
#           are multiples of 2^-11 below 2^11 (the second output: of 2^-10 below 2^12): the 22 bits of a half-float pair; the sinks
#           have two taps, opposite corners, so that their float32 sums stay below 2^13 at that quantum;
#   'bf16'  0 .. 63: |src| <= 3 * 63 + 8 = 197: 8 bits, one bf16 word; the outputs stay far below the 16 bits of a bf16 pair.
LO_FACTOR = 1.0 + 2.0 ** -11                       # 12 significant bits: hi = 1, lo = 2^-11 (times the row's power of two)
LO_QUANTUM = -11                                   # ... so an 'f16x2' program holds multiples of 2^-11, exact in float32 below 2^13
MODE_CONV_CASES = {'c64to64_1x1': dict(C=64, cout=64, k=1, epi=('plain', 'prelu_res32_out2', 'relu_out2'))}      # 'f16': ONE slab of 64
MODE_FULL_SIZE_CASES = ('c128_3x3',)               # the single pixel and the exact tile: one case per mode


def mode_frames(net, size, stride=1):
    return frames(frame_seed(size), *frame_size(size, stride)) >> net.pixel_shift


def all_cases(precision):
    return dict(CONV_CASES, **MODE_CONV_CASES) if precision in TOLERANCE_MODES else CONV_CASES


def conv_programs(case, variant, precision):
    """[(epilogue, io, sizes)] `variant` can run of CONV_CASES[case] in `precision`.  io 'f32': shortcut and outputs pinned to float32
    ('generic': the input as well); 'split': every tensor in the precision's pre-split format, where the split-role and window
    kernels take the lean drain for LEAN_EPILOGUES."""
    c = all_cases(precision)[case]
    staged = c.get('out_off', 0) % 8 == 0
    out = []
    for epi in c['epi']:
        e = EPILOGUES[epi]
        sizes = [s for s in case_sizes(case, e.get('affine'), precision)
                 if variant_eligible(variant, precision, cout=c['cout'], k=c['k'], stride=c.get('stride', 1), groups=c.get('groups', 1),
                                     staged=staged, size=s, cin=c['C'] // c.get('groups', 1))]
        for io in ('f32', 'split'):
            if io == 'split' and (precision == 'f32' or (variant == 'generic' and precision not in TOLERANCE_MODES)):
                continue                               # (the tolerance modes: the generic kernel's drains store their formats as well)
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


STAGE_DATA = dict(src_wmax=1, mags=(4, 1, 2, 1), sink_taps=None, scale2=(-2, -1, 1, 2), shift2=100)      # what rounded_net varies


def _stage(net, rng, c, e, variant, io, *, stride=1, res_from=None, res_up2=0, k_split=0, nz=3, seed_affine=True, data=None):
    """'src' -> the conv under test with epilogue `e` -> 'out' (-> 'out2'), and a sink conv behind each output.  `data`: entries of
    STAGE_DATA that differ.  net.want_formats: the storage format every named tensor is MEANT to have (assert_formats)."""
    d = dict(STAGE_DATA, **(data or {}))
    src_wmax, mags, sink_taps = d['src_wmax'], d['mags'], d['sink_taps']
    from terran_amd import lib
    C, cout, k, groups = c['C'], c['cout'], c['k'], c.get('groups', 1)
    pin = io == 'f32'
    mode = net.like                                  # whose widths, weights and frames the program has (mode_net)
    # 'f16': a TA_FMT_F16 tensor has whole 64-channel blocks, so every width and slice offset of 32 above becomes 64 (cout + 64 wide,
    # read or written at 64), and it takes no in_ch_off: the input slice is dropped.  wide = 8: selector magnitude 1 (MODE_PIXEL_SHIFT)
    blk = 64 if mode == 'f16' else 32
    wide = 8 if mode == 'f16' else 16
    off = lambda v: v // 32 * blk
    # the tolerance modes: every width a whole block (40 + 64 -> 128), so that the direct drain too meets the mode's format thrice
    wid = (lambda w: -(-w // blk) * blk) if mode in TOLERANCE_MODES else (lambda w: w)
    in_off = 32 if e.get('in_slice') and mode != 'f16' else 0
    selector(net, rng, 'src', C + in_off, halo=k // 2, wmax=src_wmax, f32=src_is_f32(variant, mode))
    kw = dict(stride=stride, groups=groups, variant=lib.CONV_VARIANTS[variant], in_ch_off=in_off, k_split=k_split, relu=bool(e.get('relu')))
    if e.get('res') is not None:
        selector(net, rng, 'shortcut', wid(cout + blk), k=3, halo=2, wmax=wide, f32=pin, stride=2 if res_up2 else stride)
        kw.update(res='shortcut', res_ch_off=off(e['res']), res_up2=res_up2)
    out_total, out_off = c.get('out_total', cout + 2 * blk if e.get('out_slice') else cout), c.get('out_off', blk if e.get('out_slice') else 0)
    if out_total != cout:
        selector(net, rng, 'out', out_total, k=3, halo=1, wmax=wide, f32=pin, stride=stride)      # every channel written before
    else:
        net.tensor('out', cout, 1, f32=pin)
    if e.get('out2') is not None:
        if e['out2']:
            selector(net, rng, 'out2', wid(cout + blk), k=3, halo=1, wmax=wide, f32=pin, stride=stride)
        else:
            net.tensor('out2', cout, 1, f32=pin)
        kw.update(out2='out2', out2_ch_off=off(e['out2']), scale2=rng.choice(list(d['scale2']), cout).astype(np.float64),
                  shift2=rng.integers(-d['shift2'], d['shift2'] + 1, cout).astype(np.float64))
    if e.get('prelu'):
        kw['prelu'] = rng.choice([-2, -1, 0, 2, 3], cout).astype(np.float64)
    if e.get('affine'):
        kw['in_affine'] = (rng.choice([-1, 1, 2], C).astype(np.float64), rng.integers(-8, 9, C).astype(np.float64))
    W, b = stage_weights(rng, cout, C // groups, k, nz=nz, mags=mags, ranges=max(k_split, 1))
    if mode == 'f16x2':                              # every output channel: one weight with a non-zero lo half
        for o in range(cout):
            ci, ky, kx = np.argwhere(W[o])[0]
            if src_wmax > 1 and ci % 4 < 2:              # 'rounded': the lo-bearing weight sits on a weak channel of 'src' (selector_weights)
                W[o, ci - ci % 4 + 2, ky, kx], W[o, ci, ky, kx] = W[o, ci, ky, kx], 0.0
                ci += 2 - ci % 4
            W[o, ci, ky, kx] *= LO_FACTOR
    net.conv('src', 'out', W, b, out_ch_off=out_off, **kw)
    # the sinks are pinned as well, to another kernel than the one under test: the launch counts then say which conv ran where
    # (40 or 72 channels are no whole K slabs: those sinks are the generic kernel's, as the conv under test is)
    net.sink_variant = sv = 'pipe64' if variant != 'pipe64' and cout % 32 == 0 else ('generic' if pin else 'split_1x4')
    if mode == 'f16' and not pin:                    # a TA_FMT_F16 tensor is read by the split-role kernels alone
        sv = net.sink_variant = 'split_1x4_w2' if variant == 'split_1x4' else 'split_1x4'
    sink_taps = sink_taps or (X2_SINK_TAPS if mode == 'f16x2' else range(9))
    sink_mode = SISTER_MODE.get(net.precision)                # (module text: the sinks of 'f16x2' / 'bf16' read both words)
    # (a width that is no whole block of the mode's format stays float32 though nothing pins it: that sink is the generic kernel's)
    w2 = wid(cout + off(e['out2'])) if e.get('out2') else cout       # the second sink reads the whole of 'out2'
    svs = [sv if pin or w % blk == 0 else 'generic' for w in [out_total] + ([w2] if e.get('out2') is not None else [])]
    sink(net, rng, 'out', 'after', out_total, variant=lib.CONV_VARIANTS[svs[0]], precision=sink_mode, taps=sink_taps)
    if e.get('out2') is not None:
        sink(net, rng, 'out2', 'after2', w2, variant=lib.CONV_VARIANTS[svs[1]], precision=sink_mode, taps=sink_taps)
    n_sel = sum(1 for s in net.steps if s[1] == 'input')
    net.counts = {variant: 1}                                       # what Context.conv_counts() must show after one forward
    for v, n in [('generic', n_sel)] + [(v, 1) for v in svs]:
        net.counts[v] = net.counts.get(v, 0) + n
    if lean_expected(variant, net.precision, e, io, k_split):
        net.counts['lean_epilogue'] = 1
    net.names = [n for n in ('src', 'shortcut', 'out', 'out2', 'after', 'after2') if n in net.tid]
    # the formats meant: 'src' float32 for the kernels that read nothing else and off the 8-channel grid, the mode's own format
    # otherwise; shortcut and outputs float32 when pinned or no whole blocks wide; the sinks' outputs float32
    own = pack.SPLIT_FMT[pack.PRECISIONS[net.precision]]
    staged = (out_off | kw.get('res_ch_off', 0) | kw.get('out2_ch_off', 0)) % 8 == 0
    chans = {n: net.P.tensors[net.tid[n]][0] for n in net.names}
    net.want_formats = {n: pack.FMT_F32 if n.startswith('after') or pin or chans[n] % blk else own for n in net.names}
    net.want_formats['src'] = pack.FMT_F32 if src_is_f32(variant, mode) or not staged or (mode == 'f16' and groups > 1) else own
    return net


def assert_formats(net):
    """The packer gives every named tensor the format the program was built for (tensor_formats(), not an assumption): a program
    listed for a drain's TA_FMT_F16 / pre-split store does meet that store."""
    f = net.P.tensor_formats()
    got = {n: f[net.tid[n]] for n in net.names}
    assert got == net.want_formats, (net.precision, got, net.want_formats)
    return got


def mode_net(precision, like=None, family='exact'):
    """A Net whose frames are shifted as the mode's exactness rule needs (MODE_PIXEL_SHIFT; 0 outside the tolerance modes, and in
    the 'rounded' family).  like: the program of that mode -- widths, weights, frames, sink taps -- with every op in `precision`."""
    net = Net(precision, pixel_shift=MODE_PIXEL_SHIFT.get(like or precision, 0) if family == 'exact' else 0, family=family)
    net.like = like or precision
    return net


X2_SINK_TAPS = (0, 8)


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def epilogue_net(precision, case, variant, epi, io='f32', like=None):
    """selector (3 -> C) -> 'src'; a 3x3 selector -> 'shortcut' (32 channels wider than cout, halo 2); the conv of CONV_CASES[case]
    with EPILOGUES[epi], pinned to `variant` -> 'out' (halo 1; a slice of a tensor a 3x3 selector has written where the epilogue or
    the case says so) and 'out2'; sink convs 'after' / 'after2' read both with their halos.  The weights depend on (case, epi) alone:
    every variant, io and precision of a case computes the same numbers.  like='f16x2' with precision 'f16x3': the two-product mode's
    program (lo-bearing weights, 11-bit activations) in the three-product mode, whose 'out' it then shares bit for bit."""
    c = all_cases(like or precision)[case]
    return _stage(mode_net(precision, like), np.random.default_rng(_seed('epilogue', case, epi)), c, EPILOGUES[epi], variant, io, stride=c.get('stride', 1))


# ---- the 'rounded' family: the same stage on operands or results that exceed the mode's bit counts (module text) --------------------
# Frames of the whole 0 .. 255.  'f16': the sums reach several thousand, so the TA_FMT_F16 stores of 'out' / 'out2' round to 11 bits (a
# float32-pinned 'out' is then rounded when the sink forms its operand); 'bf16': |src| reaches 773, 10 bits, so the conv under test
# reads bf16_rne(src); 'f16x2': 'src' comes from a selector of magnitude 8 on every fourth channel (|src| <= 6184: 13 bits; <= 773 on
# channels 2 and 3 of four) and is read as x_hi = f16_rne(src 2^a) 2^-a, a from the packed program's exponents; each output channel has
# two weights of magnitude 1, the lo-bearing one on a weak channel, and no PReLU slope multiplies the sums: 6184 + 773 + 50 < 2^13 at
# the quantum 2^-11, exact in float32; what the half-float pair of 'out' / 'out2' cannot hold (22 bits) is rounded by the reference
# as the store rounds it; each sink has ONE tap, the corner that reads the halo; the second output has scales of +-1 and shifts within
# 40 (7007 + 40 < 2^13).  The 40-channel case is the generic kernel's direct drain; K in 2 and 4 ranges ends in splitk_reduce_kernel:
# with the staged and the lean drain of the other programs, every one of the four stores rounds something.
ROUNDED_CASES = ('c64_3x3', 'c128_3x3', 'c64to64_1x1', 'c128to40in192_1x1')
ROUNDED_EPILOGUES = {'f16': ('plain', 'prelu_res32_out2', 'res0_out2_slice'), 'bf16': ('plain', 'prelu_res32_out2', 'res0_out2_slice'),
                     'f16x2': ('plain', 'relu_out2')}
ROUNDED_KSPLIT = (('c128_3x3', 'res0_out2_slice', 2), ('c128_3x3', 'prelu', 4))      # (case, epilogue, K ranges) on KSPLIT_VARIANTS
ROUNDED_SIZES = ((3, 5, 3), (3, 9, 10))


def rounded_net(precision, case, variant, epi, io='split', k_split=0):
    c = all_cases(precision)[case]
    x2 = precision == 'f16x2'
    data = dict(src_wmax=8, mags=(1, 1, 1, 1), sink_taps=(0,), scale2=(-1, 1), shift2=40) if x2 else None
    return _stage(mode_net(precision, family='rounded'), np.random.default_rng(_seed('rounded', case, epi, k_split)), c, EPILOGUES[epi], variant, io,
                  nz=(2 if x2 else 3) + (2 if k_split else 0), k_split=k_split, data=data)


def rounded_programs(case, variant, precision):
    """[(epilogue, io, K ranges)] of ROUNDED_CASES[case] that `variant` can run: pre-split io wherever the kernel has it."""
    c = all_cases(precision)[case]
    if not variant_eligible(variant, precision, cout=c['cout'], k=c['k'], cin=c['C'], size=ROUNDED_SIZES[-1], staged=c.get('out_off', 0) % 8 == 0):
        return []
    out = [(epi, 'split', 0) for epi in ROUNDED_EPILOGUES[precision]]
    if variant in KSPLIT_VARIANTS and precision != 'f16x2':       # ('f16x2': four weights of up to 6184 would pass 2^13 at its quantum)
        out += [(epi, 'split', ks) for cs, epi, ks in ROUNDED_KSPLIT if cs == case]
    return out


UP2_CASES = ('c64_3x3', 'c128_3x3')
UP2_EPILOGUES = {'relu_res0': dict(relu=True, res=0), 'res32': dict(res=32), 'res32_out2': dict(res=32, out2=0)}


def up2_net(precision, case, variant, epi, io='f32'):
    """As epilogue_net, but 'shortcut' comes from a STRIDE-2 3x3 selector on the same frames -- ceil(h / 2) x ceil(w / 2) -- and the
    conv under test reads it at (y >> 1, x >> 1) (RetinaFace's FPN merge, pack/retinaface.py)."""
    return _stage(mode_net(precision), np.random.default_rng(_seed('up2', case, epi)), CONV_CASES[case], UP2_EPILOGUES[epi], variant, io, res_up2=1)


def up2_programs(case, variant, precision):
    c = CONV_CASES[case]
    out = []
    for epi in UP2_EPILOGUES:
        sizes = tuple(s for s in case_sizes(case, False, precision) if variant_eligible(variant, precision, cout=c['cout'], k=c['k'], size=s, cin=c['C']))
        out += [(epi, io, sizes) for io in ('f32', 'split') if sizes and not (io == 'split' and (precision == 'f32' or (variant == 'generic' and precision not in TOLERANCE_MODES)))]
    return out


KSPLIT_CASES = {'c256_3x3': dict(C=256, cout=128, k=3), 'c512_1x1': dict(C=512, cout=128, k=1)}
KSPLIT_EPILOGUES = {'relu': dict(relu=True), 'prelu': dict(prelu=True), 'res32': dict(res=32), 'res0_out2_slice': dict(res=0, out2=32),
                    'affine_prelu': dict(prelu=True, affine=True)}                  # in_affine: 3x3 only, no second output (Program.conv)
KSPLIT_VARIANTS = ('split_2x2', 'split_2x4', 'split_1x4')                            # the 3-stage split-role kernels know K ranges
KSPLITS = (2, 4)


def ksplit_net(precision, case, variant, epi, k_split, io='f32'):
    """As epilogue_net with K cut in `k_split` ranges: the kernels write raw partial sums, splitk_reduce_kernel runs the whole epilogue.
    Every output channel has a weight in every range."""
    return _stage(mode_net(precision), np.random.default_rng(_seed('ksplit', case, epi, k_split)), KSPLIT_CASES[case], KSPLIT_EPILOGUES[epi],
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
DWPW_CASES = ((64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (32, 32, 1), (32, 64, 2), (96, 40, 1), (64, 24, 1),
              # more than 256 input channels (dwpw_table_loader: the depthwise table's tail loop); the last: two cout tiles as well
              (320, 64, 1), (1024, 64, 1), (1024, 128, 1), (320, 256, 1))
# frames (h, w) of two images, or (n, h, w).  At stride 1 the block's map is the frame's: M = 70 and 288 (several images in a partial
# tile); 64, 128, 256 (whole tiles of 64 and of 128 pixels); 63 | 65 and 127 | 129 (one pixel either side); 126 (2 x 7 x 9: tile 0 of
# 64 holds image 0 and ONE pixel of image 1, both of an odd Ho Wo) and 130 (2 x 5 x 13: the 128-pixel tile likewise)
DWPW_SHAPES = ((5, 7), (9, 16), (4, 8), (8, 8), (8, 16), (3, 3, 7), (1, 5, 13), (1, 1, 127), (1, 3, 43), (7, 9), (5, 13))
DWPW_BIG_C_SHAPES = ((5, 7),)                    # what the cases of more than 256 input channels run: M = 70
# (C, cout, stride) -> frames: more than 8 pixel tiles, so that ta_xcd_tile deals whole rounds (base >= 1) and a remainder -- what
# every launch of the real detector does.  2 x 23 x 23: M = 1058 = 9 tiles of 128, 17 of 64; 2 x 45 x 48 at stride 2: an odd x even
# map of 23 x 24, M = 1104 = 9 tiles of 128, 18 of 64
DWPW_MANY_TILES = {(64, 64, 1): (2, 23, 23), (128, 128, 1): (2, 23, 23), (64, 24, 1): (2, 23, 23), (64, 128, 2): (2, 45, 48), (32, 64, 2): (2, 45, 48)}
RFSTEM_SHAPES = ((1, 27, 123), (1, 29, 125), (2, 57, 249), (1, 5, 7), (1, 56, 248), (1, 31, 126), (3, 16, 16))
# The fused front's own geometry (rfstem_fused_geometry: 6 x 30 tiles of the quarter-resolution map), what each shape is for:
#   1 x 21 x 117  exactly one tile (oh, ow = 6, 30), 3 W mod 4 = 3, mh = 11 and mw = 59 odd: the tile's last row and column read
#                 row 11 / column 59 of the 16-channel map, which lie outside it
#   2 x 23 x 118  one tile, 3 W mod 4 = 2, mh = 12 even, mw = 59 odd; the second image starts 2 bytes off a dword
#   2 x 23 x 119  one tile, 3 W mod 4 = 1, mh = 12, mw = 60 even; the second image starts 3 bytes off
#   1 x 24 x 120  one tile, 3 W mod 4 = 0, mh = 12, mw = 60: the largest frame of one tile
#   2 x 25 x 121  one output row and column more than a tile (7 x 31); second image 3 bytes off
#   1 x 43 x 235  one row and column less than two tiles (11 x 59)
#   1 x 48 x 240  exactly 2 x 2 tiles
#   2 x 47 x 245  the smallest width at which a tile (column 1 of 3) copies its window unmasked (x_inside)
#   3 x 49 x 244  one pixel narrower: no tile is x_inside; three tile rows (oh = 13)
#   1 x 5 x 7     a frame smaller than one window
RFSTEM_FUSED_SHAPES = ((1, 21, 117), (2, 23, 118), (2, 23, 119), (1, 24, 120), (2, 25, 121), (1, 43, 235), (1, 48, 240), (2, 47, 245),
                       (3, 49, 244), (1, 5, 7))
RFSTEM_ALL_SHAPES = RFSTEM_SHAPES + tuple(s for s in RFSTEM_FUSED_SHAPES if s not in RFSTEM_SHAPES)


def dwpw_shapes(C, cout=None, stride=None):
    """The (n, h, w) frames test_dwpw runs a case of DWPW_CASES on."""
    return tuple(s if len(s) == 3 else (2,) + s for s in (DWPW_BIG_C_SHAPES if C > 256 else DWPW_SHAPES))


# ---- the tiling of the two detector kernels, mirrored from the .hip files (tests/test_exact_programs_cpu.py proves from these that
# ---- the lists above reach every path they are listed for) ------------------------------------------------------------------------
RFS_OY, RFS_OX = 6, 30                           # csrc/layers.hip:236-237: output tile of rf_stem_kernel<true>
RFS_IXB = (2 * (62 + 2) + 1) * 3                 # csrc/layers.hip:210-214: bytes per window row (387)


def rfstem_fused_geometry(h, w):
    """rf_stem_kernel<true> on h x w frames (csrc/layers.hip:551-552, 572: ta_launch_rfstem; 247-249, 262: the kernel).  -> dict:
    mh, mw the 16-channel half-resolution map; oh, ow the quarter-resolution output; tiles_y, tiles_x the grid; origin(by, bx) the
    frame (row, column) of a tile's window; x_inside(bx) whether the tile copies its window rows as unmasked dwords."""
    mh, mw = (h + 1) // 2, (w + 1) // 2
    oh, ow = (mh + 1) // 2, (mw + 1) // 2

    def origin(by, bx):
        ty0, tx0 = 2 * RFS_OY * by - 1, 2 * RFS_OX * bx - 1          # layers.hip:247-248 (FUSE)
        return 2 * (ty0 - 1) - 1, 2 * (tx0 - 1) - 1                  # layers.hip:249: iy0, ix0 = 24 by - 5, 120 bx - 5

    def x_inside(bx):
        ix0 = origin(0, bx)[1]
        return ix0 >= 0 and ix0 * 3 + RFS_IXB + 3 <= w * 3          # layers.hip:262

    return dict(mh=mh, mw=mw, oh=oh, ow=ow, tiles_y=-(-oh // RFS_OY), tiles_x=-(-ow // RFS_OX), origin=origin, x_inside=x_inside)


def dwpw_tile(cout, lean):
    """(BN, BM) of the block's launch: csrc/conv_dwpw.hip:452-454 with :163 (rf_dwpw_kernel, `lean`), :456-462 with :21-22 (conv_dwpw)."""
    coutp = -(-cout // 32) * 32
    if coutp % 128 == 0:
        return (128, 64) if lean else (128, 128)
    if coutp % 64 == 0:
        return (64, 64) if lean else (64, 128)
    return 32, 128


def xcd_tile(n_pt, xcd, local):
    """csrc/conv_common.h:101-105: ta_xcd_tile."""
    base, rem = n_pt >> 3, n_pt & 7
    if local >= base + (1 if xcd < rem else 0):
        return -1
    return xcd * base + min(xcd, rem) + local


def dwpw_grid(cout, M, lean):
    """-> dict(BN, BM, n_ct, n_pt, blocks, tiles): csrc/conv_dwpw.hip:171-178 (:34-42) and conv_common.h:921 (ta_tile_grid);
    tiles[b] = (ct, pt) of block b, pt < 0 for a block that returns at once."""
    BN, BM = dwpw_tile(cout, lean)
    n_ct, n_pt = -(-cout // 32) * 32 // BN, -(-M // BM)
    blocks = -(-n_pt // 8) * n_ct * 8
    tiles = [((b >> 3) % n_ct, xcd_tile(n_pt, b & 7, (b >> 3) // n_ct)) for b in range(blocks)]
    return dict(BN=BN, BM=BM, n_ct=n_ct, n_pt=n_pt, blocks=blocks, tiles=tiles)


def dwpw_lean_ok(precision, C, cout):
    """csrc/conv_dwpw.hip:446-450: the f16x3 launch takes rf_dwpw_kernel (the programs here: ReLU, float32 out, n_slabs 32 == C)."""
    return precision == 'f16x3' and C % 32 == 0 and C <= 1024 and cout % 8 == 0


DWPW_TABLE_FIRST = 3 * 256                       # csrc/conv_dwpw.hip:193-200: granules the unrolled prologue loads (WG = 3 per thread)
LDS_PER_CU = 160 * 1024                          # gfx950


def dwpw_table_loader(C, row, c):
    """Which loop of rf_dwpw_kernel puts value (row, c) of the depthwise table [9 taps + bias][C] into LDS (row 9: the bias):
    -> (granule, trip); trip 0: the unrolled prologue (conv_dwpw.hip:196-200, 323-325), trip k >= 1: pass k of the tail loop (:326-327)."""
    g = (row * C + c) // 4
    return g, 0 if g < DWPW_TABLE_FIRST else 1 + (g - DWPW_TABLE_FIRST) // 256


def dwpw_lean_lds(C, cout):
    """csrc/conv_dwpw.hip:411: two stages and the table."""
    BN, BM = dwpw_tile(cout, True)
    return 2 * (BN + BM) * 32 * 4 + 40 * C

# One case per grid-stride kernel whose work items (the `total` of its ta_launch_*) just exceed the 2048 x 256 threads a launch is
# capped at, so that the loop's second trip runs: (frame h, w) and the total, for one image, float32.
GRID_CAP = 2048 * 256
SECOND_TRIP = {
    'preprocess': ((725, 724), 725 * 724),                          # n h w pixels
    'dwconv': ((257, 256), 257 * 256 * (32 // 4)),                  # n ho wo (C / 4), stride 1, C = 32
    'maxpool': ((364, 362), 182 * 181 * (64 // 4)),                 # n ho wo (C / 4) of the POOLED map, C = 64
    'copych': ((257, 256), 257 * 256 * (32 // 4)),                  # n h w (ch / 4), 32 channels copied
}
