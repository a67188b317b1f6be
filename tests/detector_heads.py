"""A detector whose heads the test paints: the program, the painters and the float64 reference (no GPU import).

`ta_retinaface_run` is the entry that ships: the network's float32 logits go straight into rf_select_kernel (cls_is_prob = 0),
which then runs its float softmax, the `fg - bg < margin` shortcut, the 16-byte cell loads with the incremental (level, y, x)
walk, the 64-bit mask of a thread's run and, past 64 anchors per run, the rescoring loop.  The real network puts a few dozen
candidates wherever it likes; this one puts every logit where the test wants it.

The program (kind MODEL_RETINAFACE, 'f32', 1 x 1 convs only):

    input (B, G, R, 0) -> 1x1 s2 + ReLU -> t2 -> 1x1 s2 -> t4 -> 1x1 s2 -> t8 -> 1x1 s2 -> t16 -> 1x1 s2 -> t32
    t8 -> 1x1 -> head8,  t16 -> 1x1 -> head16,  t32 -> 1x1 -> head32        (32 channels, halo 0, float32; no activation)

A 1 x 1 stride-2 conv maps h to ceil(h / 2), so head cell (y, x) of stride s sees pixel (s y, s x) alone.  The first conv carries
four numbers of that pixel, B, G, R and Q = max(R - 1, 0); every later chain conv passes them on, each time five channels further
up (CARRY_STEP).  A head is a linear map of (B, G, R, Q) with weights that are integers or powers of two down to 2^-6 and integer
biases: every head value is a multiple of 2^-6 far below 2^24, exact in float32 in any summation order.

What a pixel means.  X_0 = B and X_1 = G set anchor a's logit margin, R in {0, 1, 2} says WHICH level the pixel speaks to:

    fg_a - bg_a = (X_a - 128) / 64 - 8 g_l(R),    g_8 = R,   g_16 = 2 Q - R + 1 = |R - 1|,   g_32 = 2 - R

so a pixel that several levels sample (stride-32 cells are stride-16 and stride-8 cells too) passes at one of them at most and
is at least 6 below every threshold at the others.  The split into fg and bg differs per level (head_matrix).  Box deltas: dx of anchor
a comes from the OTHER anchor's byte, dy from its own, dw = dh = 0 (expf(0) in the decode); the ten landmark deltas mix both bytes
with powers of two and integer biases; signs and biases differ per level.  Pixels that no head samples are random bytes.

The reference: heads by a float64 matrix product on the sampled pixels, probabilities float32(1 / (1 + exp(-(fg - bg)))) computed
in float64, detections by oracle.retinaface_post.postprocess on those heads in the reference layout.  `reference(case, mistake)`
with a name of MISTAKES gives a deliberately wrong one (tests/test_detector_heads_cpu.py shows that each differs on a listed case).
"""
import math

import numpy as np

from oracle import retinaface_post as orp
from terran_amd import pack

STRIDES = (32, 16, 8)                     # the order of the concatenated anchors and of P.outputs
CODE = {8: 0, 16: 1, 32: 2}               # the value of R that lets a pixel pass at this level
CARRY_STEP = 5                            # each chain conv moves the four carried channels this far up (mod 32)
RF_THREADS = 1024                         # csrc/retinaface_post.hip
FAIL_TOP = 60                             # background bytes are 0 .. FAIL_TOP - 1: (59 - 128) / 64 = -1.08, under every margin in use
QUANTUM = 64.0                            # every head value times this is an integer

# d64 = 64 (fg - bg) of the classes that straddle each threshold: (fail by the shortcut or the exact test, pass)
STRADDLE = {0.5: ((-2, -1), (0, 1)),      # margin -0.01: -1/64 is skipped and fails the exact test too; 0 scores exactly 0.5
            0.3: ((-56, -55), (-54, -53)),    # logit -0.8473, margin -0.8581: -55/64 = -0.8594 is skipped, -54/64 = -0.8438 passes
            0.75: ((69, 70), (71, 72))}   # logit 1.0986, margin 1.0875: 69/64 is skipped, 70/64 = 1.0938 takes the exact test and fails it
TIE_CLASSES = (127, 112, 96)              # pass at every threshold; shared by many anchors of all levels


def margin(thr):
    """The host's shortcut bound (csrc/retinaface_post.hip: rf_postprocess_dev), in float64."""
    lg = math.log(thr / (1.0 - thr))
    return lg - 0.01 - 0.001 * abs(lg)


# ---- geometry --------------------------------------------------------------------------------------------------------------------
class Geometry:
    """Anchor bookkeeping of an (H, W) frame: per level fh, fw and the first anchor index t0; T anchors, ncell cells, and the
    kernel's split of the cells into thread runs of `perc` cells (`per` anchors)."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.fh = {s: -(-H // s) for s in STRIDES}
        self.fw = {s: -(-W // s) for s in STRIDES}
        self.t0, t = {}, 0
        for s in STRIDES:
            self.t0[s] = t
            t += 2 * self.fh[s] * self.fw[s]
        self.T, self.ncell = t, t // 2
        self.perc = -(-self.ncell // RF_THREADS)
        self.per = 2 * self.perc

    def locate(self, t):
        """anchor index -> (stride, y, x, a)"""
        s = 8 if t >= self.t0[8] else (16 if t >= self.t0[16] else 32)
        cell, a = divmod(t - self.t0[s], 2)
        y, x = divmod(cell, self.fw[s])
        return s, y, x, a

    def anchor(self, s, y, x, a):
        return self.t0[s] + 2 * (y * self.fw[s] + x) + a

    def cells(self, s):
        return self.fh[s] * self.fw[s]


# ---- the program -----------------------------------------------------------------------------------------------------------------
def _carry_pos(stage):
    """Channels of (B, G, R, Q) in the chain tensor after `stage` convs (stage 1 = t2)."""
    return [(c + CARRY_STEP * (stage - 1)) % 32 for c in range(4)]


def head_matrix(s):
    """(32, 4) weights over (B, G, R, Q) and (32,) bias of the head of stride `s`.  Channels: bg0 bg1 fg0 fg1 | anchor 0: dx dy dw dh,
    anchor 1: dx dy dw dh | anchor 0: ten landmark deltas, anchor 1: ten."""
    M, b = np.zeros((32, 4)), np.zeros(32)
    B, G, R, Q = 0, 1, 2, 3
    for a, X in ((0, B), (1, G)):
        bg, fg = a, 2 + a
        M[fg, X] = 1.0 / 64
        if s == 8:                        # fg = X / 64,              bg = 8 R + 2
            M[bg, R], b[bg] = 8, 2
        elif s == 16:                     # fg = X / 64 + 8 R - 8,    bg = 16 Q + 2
            M[fg, R], b[fg] = 8, -8
            M[bg, Q], b[bg] = 16, 2
        else:                             # fg = X / 64 + 4 R - 8,    bg = 10 - 4 R
            M[fg, R], b[fg] = 4, -8
            M[bg, R], b[bg] = -4, 10
        other = G if a == 0 else B
        sx, sy = (-1 if s == 16 else 1), (-1 if s == 32 else 1)
        M[4 + 4 * a, other], b[4 + 4 * a] = sx / 64.0, -sx * (1 + a)                 # dx: within +-3 anchor widths
        M[5 + 4 * a, X], b[5 + 4 * a] = sy / 32.0, -sy * 4                           # dy
        for k in range(5):                                                           # dw = dh = 0: channels 6, 7, 10, 11 stay zero
            M[12 + 10 * a + 2 * k, other], b[12 + 10 * a + 2 * k] = sx * 2.0 ** -(k + 2), k + s // 8
            M[13 + 10 * a + 2 * k, X], b[13 + 10 * a + 2 * k] = sy * 2.0 ** -(6 - k), -k - a
    return M, b


def program():
    """The pack.Program (it does not depend on the frame size).  head8 is the last tensor: in the plan's arena head32 and head16,
    the two levels the selection walks out of, are followed by another tensor."""
    P = pack.Program(pack.MODEL_RETINAFACE, 'f32')
    t_in = P.tensor(4, 1, name='input')
    P.input_tensor = t_in
    chain = [P.tensor(32, 0, name=name) for name in ('t2', 't4', 't8', 't16', 't32')]
    heads = {s: P.tensor(32, 0, name='head%d' % s, f32=True) for s in STRIDES}
    src = t_in
    for stage, dst in enumerate(chain, 1):
        pos = _carry_pos(stage)
        if stage == 1:                    # (B, G, R) -> B, G, R, max(R - 1, 0); the ReLU leaves the three bytes as they are
            W, b = np.zeros((32, 3, 1, 1)), np.zeros(32)
            for c in range(3):
                W[pos[c], c] = 1
            W[pos[3], 2], b[pos[3]] = 1, -1
            P.conv(src, dst, W, b, stride=2, pad=0, act=pack.ACT_RELU)
        else:
            W, prev = np.zeros((32, 32, 1, 1)), _carry_pos(stage - 1)
            for c in range(4):
                W[pos[c], prev[c]] = 1
            P.conv(src, dst, W, np.zeros(32), stride=2, pad=0)
        src = dst
        s = 1 << stage
        if s in CODE:
            M, b = head_matrix(s)
            W = np.zeros((32, 32, 1, 1))
            W[:, pos, 0, 0] = M
            P.conv(src, heads[s], W, b, pad=0)
    P.outputs = [heads[32], heads[16], heads[8]]
    return P


# ---- frames ----------------------------------------------------------------------------------------------------------------------
class Painter:
    """One frame (H, W, 3) uint8 RGB.  Every byte starts random; the sampled pixels (both coordinates multiples of 8) get B, G below
    FAIL_TOP and a random level code in R, so nothing passes until `set` says so."""

    def __init__(self, geo, seed):
        self.geo = geo
        self.rng = rng = np.random.default_rng(seed)
        self.fr = rng.integers(0, 256, (geo.H, geo.W, 3), dtype=np.uint8)
        gy, gx = self.fr[::8, ::8].shape[:2]
        self.fr[::8, ::8, 0] = rng.integers(0, 3, (gy, gx))                      # R
        self.fr[::8, ::8, 1:] = rng.integers(0, FAIL_TOP, (gy, gx, 2))           # G, B
        self.owner = {}                   # pixel -> stride that claimed it
        self.live = {}                    # anchor index -> d64 (passing or not)

    def free(self, s, y, x):
        return self.owner.get((s * y, s * x), s) == s

    def set(self, t, d64):
        """64 (fg - bg) of anchor t becomes d64 (-128 .. 127); the pixel now speaks to t's level."""
        s, y, x, a = self.geo.locate(t)
        py, px = s * y, s * x
        assert self.owner.setdefault((py, px), s) == s, 'pixel (%d, %d) already speaks to stride %d' % (py, px, self.owner[py, px])
        assert -128 <= d64 <= 127
        self.fr[py, px, 0] = CODE[s]
        self.fr[py, px, 2 - a] = 128 + d64                                     # a = 0: B (RGB byte 2), a = 1: G (byte 1)
        self.live[t] = d64


def _pick(rng, classes, weights=None):
    return int(classes[rng.choice(len(classes), p=weights)])


def paint_exact_count(geo, seed, C, thr, first_of=16, mix=(0.1, 0.3, 0.6), near_fail=24):
    """Exactly C anchors pass.  In order of priority: anchor 1 of the last stride-32 cell beside a failing anchor 0; both anchors of
    the first cell of level `first_of` (the pixel (0, 0) can speak to one level only); anchor 0 of the last stride-16 cell beside a
    failing anchor 1; the very last anchor; then runs of consecutive cells over all three levels in the shares `mix`, with both or
    one anchor of a cell passing.  Passing anchors draw their class from TIE_CLASSES (most) and the passing straddle classes,
    failing ones beside them and `near_fail` further cells from the failing straddle classes."""
    p = Painter(geo, seed)
    rng = p.rng
    fails, passes = STRADDLE[thr]
    pass_classes = TIE_CLASSES + tuple(passes)
    pass_w = np.array([0.35, 0.25, 0.2] + [0.2 / len(passes)] * len(passes))
    want = []                             # (anchor, passes?)
    last32 = geo.anchor(32, geo.fh[32] - 1, geo.fw[32] - 1, 0)
    last16 = geo.anchor(16, geo.fh[16] - 1, geo.fw[16] - 1, 0)
    first = geo.anchor(first_of, 0, 0, 0)
    want += [(last32 + 1, True), (last32, False), (first, True), (first + 1, True), (last16, True), (last16 + 1, False),
             (geo.T - 1, True), (geo.T - 2, False)]
    n = 0
    for t, ok in want:
        if ok and n == C:
            continue
        s, y, x, _ = geo.locate(t)
        if not p.free(s, y, x):           # (a frame so small that two of these share a pixel)
            continue
        p.set(t, _pick(rng, pass_classes, pass_w) if ok else _pick(rng, fails))
        n += ok
    quota = {32: int(mix[0] * C), 16: int(mix[1] * C)}
    for s in (32, 16):                    # no level takes more than a third of its anchors: pixels stay free for the finer ones
        quota[s] = min(quota[s], 2 * geo.cells(s) // 3)
    for s in STRIDES:
        target = n + quota[s] if s != 8 else C
        target = min(target, C)
        guard = 0
        while n < target:
            guard += 1
            assert guard < 200000, 'the frame cannot hold %d passing anchors' % C
            c0, run = int(rng.integers(0, geo.cells(s))), int(rng.integers(1, 9))
            for cell in range(c0, min(c0 + run, geo.cells(s))):
                if n == target:
                    break
                y, x = divmod(cell, geo.fw[s])
                t = geo.t0[s] + 2 * cell
                if t in p.live or t + 1 in p.live or not p.free(s, y, x):
                    continue
                kind = int(rng.integers(0, 3)) if target - n >= 2 else int(rng.integers(1, 3))      # both, a0 only, a1 only
                for a in (0, 1):
                    ok = kind == 0 or kind == 1 + a
                    p.set(t + a, _pick(rng, pass_classes, pass_w) if ok else _pick(rng, fails + (-100, -90)))
                    n += ok
    for _ in range(near_fail):            # cells that speak to their level and fail just below the threshold
        s = STRIDES[int(rng.integers(0, 3))]
        cell = int(rng.integers(0, geo.cells(s)))
        y, x = divmod(cell, geo.fw[s])
        t = geo.t0[s] + 2 * cell
        if t in p.live or t + 1 in p.live or not p.free(s, y, x):
            continue
        p.set(t, _pick(rng, fails))
        p.set(t + 1, _pick(rng, fails))
    assert n == C
    return p


def paint_offset(geo, seed, thr, offsets=(63,)):
    """Only the anchors at `offsets` of each thread's run pass (thread k's run starts at anchor k * per), wherever the pixel is
    still free; the anchor beside each fails just below the threshold."""
    p = Painter(geo, seed)
    fails, passes = STRADDLE[thr]
    pass_classes = TIE_CLASSES + tuple(passes)
    for k in range(RF_THREADS):
        for o in offsets:
            t = k * geo.per + o
            if o >= geo.per or t >= geo.T:
                continue
            s, y, x, a = geo.locate(t)
            if (t ^ 1) in p.live or not p.free(s, y, x):
                continue
            p.set(t, pass_classes[(k + o) % len(pass_classes)])
            p.set(t ^ 1, fails[k % len(fails)])
    return p


def paint_crossing_runs(geo, seed, C, thr, first_of=16):
    """per > 64: the thread runs that contain the two level boundaries pass almost everywhere (two cells of three fail on one
    anchor; the pixel (0, 0) speaks to level `first_of`), the anchors at offsets 62 .. per - 1 of every eighth run pass, and random
    runs fill up to exactly C."""
    p = Painter(geo, seed)
    rng = p.rng
    fails, passes = STRADDLE[thr]
    pass_classes = TIE_CLASSES + tuple(passes)
    n = 0

    def cell_set(t, kind):
        nonlocal n
        s, y, x, _ = geo.locate(t)
        if t in p.live or t + 1 in p.live or not p.free(s, y, x):
            return
        for a in (0, 1):
            ok = kind == 0 or kind == 1 + a
            if ok and n == C:
                ok = False
            p.set(t + a, _pick(rng, pass_classes) if ok else _pick(rng, fails))
            n += ok
    for s in (first_of, 24 - first_of):   # the run that holds the first anchor of level s, and its neighbours
        k = geo.t0[s] // geo.per
        for t in range(max(k - 1, 0) * geo.per, min((k + 2) * geo.per, geo.T), 2):
            cell_set(t, (t // 2) % 3)
    for k in range(0, RF_THREADS, 8):
        for t in range(k * geo.per + 62, min((k + 1) * geo.per, geo.T), 2):
            cell_set(t, 0)
    guard = 0
    while n < C:
        guard += 1
        assert guard < 200000
        t0 = 2 * int(rng.integers(0, geo.ncell))
        for t in range(t0, min(t0 + 2 * int(rng.integers(1, 9)), geo.T), 2):
            cell_set(t, int(rng.integers(0, 3)) if C - n >= 2 else int(rng.integers(1, 3)))
    assert n == C
    return p


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    """name, frame size, thresholds and one painter call per image; `counts`: the candidates each image is meant to have (None:
    whatever the painter could place -- then `at_least` says how many it must be); `regime`: 'short' (per < 64), 'full' (per == 64)
    or 'rescored' (per > 64)."""

    def __init__(self, name, H, W, thr, nms, images, counts, regime='short', at_least=None):
        self.name, self.H, self.W, self.thr, self.nms = name, H, W, thr, nms
        self.images, self.counts, self.regime, self.at_least = images, counts, regime, at_least
        self.geo = Geometry(H, W)
        self.N = len(images)
        self._painters = self._ref = None

    def painters(self):
        if self._painters is None:
            self._painters = [fn(self.geo, 1000 * i + 7, *args, **kw) for i, (fn, args, kw) in enumerate(self.images)]
        return self._painters

    def frames(self):
        return np.stack([p.fr for p in self.painters()])


def _exact(name, C, thr, nms, H=640, W=640, **kw):
    return Case(name, H, W, thr, nms, [(paint_exact_count, (C, thr), kw)], [C])


CASE_LIST = [
    # 640 x 640: 16 800 anchors, perc = 9.  The counts cross the all-empty return, partial and full 64-blocks of the suppression
    # matrix, the matrix / loop switch (1024) and the LDS / global sort switch (8192)
    _exact('c0', 0, 0.5, 0.4), _exact('c1', 1, 0.5, 0.4), _exact('c63', 63, 0.3, 0.4, first_of=8), _exact('c64', 64, 0.5, 0.2),
    _exact('c65', 65, 0.75, 0.4), _exact('c1023', 1023, 0.5, 0.4, first_of=8), _exact('c1024', 1024, 0.3, 0.2),
    _exact('c1025', 1025, 0.75, 0.4), _exact('c8192', 8192, 0.5, 0.4, first_of=8), _exact('c8193', 8193, 0.3, 0.4),
    Case('batch3', 640, 640, 0.5, 0.4, [(paint_exact_count, (65, 0.5), {}), (paint_exact_count, (0, 0.5), {}),
                                        (paint_exact_count, (1025, 0.5), dict(first_of=8))], [65, 0, 1025]),
    # 1248 x 1280: 32 760 cells, perc = 32, per = 64: offset 63 is bit 63 of the run's mask
    Case('per64_offset63', 1248, 1280, 0.5, 0.2, [(paint_offset, (0.5,), {})], None, 'full', at_least=900),
    # 1280 x 1288: 33 880 cells, perc = 34, per = 68: the rescoring loop; 3 000 candidates take the NMS loop, 700 the matrix
    Case('per68_rescored', 1280, 1288, 0.3, 0.4, [(paint_crossing_runs, (3000, 0.3), {}), (paint_crossing_runs, (700, 0.3), dict(first_of=8))],
         [3000, 700], 'rescored'),
    Case('per68_offsets', 1280, 1288, 0.75, 0.2, [(paint_offset, (0.75,), dict(offsets=(0, 63, 64, 67)))], None, 'rescored', at_least=3000),
    # an odd small frame: ceil head shapes, short last rows, perc = 1
    Case('odd_101x150', 101, 150, 0.3, 0.2, [(paint_exact_count, (40, 0.3), dict(near_fail=6)),
                                             (paint_exact_count, (13, 0.3), dict(first_of=8, near_fail=6))], [40, 13]),
]
CASES = {c.name: c for c in CASE_LIST}


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def heads64(geo, frames):
    """{stride: (N, 32, fh, fw) float64}: the matrix product on the sampled pixels."""
    out = {}
    for s in STRIDES:
        px = frames[:, ::s, ::s, ::-1].astype(np.float64)                      # (N, fh, fw, 3) as B, G, R
        assert px.shape[1:3] == (geo.fh[s], geo.fw[s])
        v = np.concatenate([px, np.maximum(px[..., 2:3] - 1.0, 0.0)], axis=-1)
        M, b = head_matrix(s)
        out[s] = np.moveaxis(v @ M.T + b, -1, 1)
    return out


def reference_layout(heads):
    """The nine arrays oracle.retinaface_post takes: per stride cls probabilities (N, 4, fh, fw), bbox (N, 8, ..), landmarks (N, 20, ..).
    The probabilities are float32(1 / (1 + exp(-(fg - bg)))) in float64 (bg: 1 minus that, unused by the oracle)."""
    out = []
    for s in STRIDES:
        h = heads[s]
        d = h[:, 2:4] - h[:, 0:2]
        fg = 1.0 / (1.0 + np.exp(-d))
        out += [np.concatenate([1.0 - fg, fg], axis=1).astype(np.float32), h[:, 4:12].astype(np.float32), h[:, 12:32].astype(np.float32)]
    return out


def margins64(geo, heads):
    """(N, T) fg - bg in anchor order, float64."""
    return np.concatenate([(heads[s][:, 2:4] - heads[s][:, 0:2]).transpose(0, 2, 3, 1).reshape(heads[s].shape[0], -1) for s in STRIDES], axis=1)


MISTAKES = ('margin_wrong_side', 'offset63_dropped', 'level_hop_late', 'ties_descending')


def _passing(case, d, scores, mistake):
    """(T,) bool: the anchors a selection with `mistake` sends on to the sort."""
    geo, thr = case.geo, case.thr
    ok = scores >= np.float32(thr)
    if mistake == 'margin_wrong_side':                    # the slack added to logit(threshold) instead of taken off, and `<=`
        lg = math.log(thr / (1.0 - thr))
        ok &= ~(d <= lg + 0.01 + 0.001 * abs(lg))
    elif mistake == 'offset63_dropped':                   # `o < 63` in the mask of a run (runs of more than 64 are scored again)
        if geo.per <= 64:
            ok[np.arange(geo.T) % geo.per == 63] = False
    elif mistake == 'level_hop_late':
        # the hop to the next level tested one cell late: inside a run that crosses a boundary, the next level's first cell is read
        # from past the end of the old level (taken as failing) and every later cell of the run one cell early
        true = ok.copy()
        for s in (16, 8):
            b = geo.t0[s] // 2                            # first cell of level s
            k = b // geo.perc
            c0, c1 = k * geo.perc, min((k + 1) * geo.perc, geo.ncell)
            if c0 < b:
                ok[2 * b:2 * b + 2] = False
                ok[2 * b + 2:2 * c1] = true[2 * b:2 * c1 - 2]
    return ok


def select(case, scores, boxes, lmks, d, mistake=None):
    """oracle.retinaface_post.select with the candidate set and the tie order open to a mistake."""
    cand = np.nonzero(_passing(case, d, scores, mistake))[0]
    if cand.size == 0:
        return []
    if mistake == 'ties_descending':
        cand = cand[::-1]
    cand = cand[np.argsort(-scores[cand], kind='stable')]
    keep = orp.nms(boxes[cand], case.nms)
    return [{'bbox': boxes[i].copy(), 'landmarks': lmks[i].copy(), 'score': scores[i]} for i in cand[keep]]


def reference(case, mistake=None):
    """-> dict(heads: {stride: float64}, d: (N, T) margins, scores (N, T) float32, dets: list[N] of list[dict]).  Without a
    mistake the detections are oracle.retinaface_post.postprocess's own; the result is cached on the case."""
    if mistake is None and case._ref is not None:
        return case._ref
    heads = heads64(case.geo, case.frames())
    nine = reference_layout(heads)
    d = margins64(case.geo, heads)
    scores, boxes, lmks = orp.decode_outputs(nine, case.H, case.W)
    if mistake is None:
        dets = orp.postprocess(nine, case.H, case.W, case.thr, case.nms)
    else:
        dets = [select(case, scores[i], boxes[i], lmks[i], d[i], mistake) for i in range(case.N)]
    out = dict(heads=heads, d=d, scores=scores, boxes=boxes, lmks=lmks, dets=dets)
    if mistake is None:
        case._ref = out
    return out


def same_detections(a, b):
    """Exact equality of two lists (per image) of detection lists."""
    if [len(x) for x in a] != [len(x) for x in b]:
        return False
    return all(np.array_equal(p['bbox'], q['bbox']) and np.array_equal(p['landmarks'], q['landmarks']) and p['score'] == q['score']
               for x, y in zip(a, b) for p, q in zip(x, y))
