import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def unflatten(counts, *arrays):
    out, o = [], 0
    for c in counts:
        out.append([tuple(a[o + i] for a in arrays) for i in range(int(c))])
        o += int(c)
    return out


def tracking_scenario(seed, n_frames=60):
    """Seeded detection sequences for the SORT tests: a handful of faces moving with constant velocity plus jitter,
    born and retired at random frames, randomly missed, occasionally crossing; a few degenerate boxes (zero height ->
    NaN state -> tracker deletion, face.py:374-381) and fast-shrinking boxes (negative area guard, face.py:196-197).
    Each face dict carries '_i' (its index within the frame) so outputs can be traced back to inputs."""
    rng = np.random.default_rng(seed)
    n_obj = int(rng.integers(3, 7))
    objs = []
    for _ in range(n_obj):
        birth = int(rng.integers(0, n_frames // 2))
        death = int(rng.integers(birth + 5, n_frames + 10))
        c = rng.uniform(100, 900, 2)
        v = rng.uniform(-12, 12, 2)
        wh = rng.uniform(40, 160, 2)
        shrink = rng.uniform(0.93, 1.03)
        objs.append((birth, death, c, v, wh, shrink))
    frames = []
    for t in range(n_frames):
        faces = []
        for (birth, death, c, v, wh, shrink) in objs:
            if not (birth <= t < death) or rng.random() < 0.12:
                continue
            k = t - birth
            cc = c + v * k + rng.normal(0, 1.5, 2)
            w, h = wh * (shrink ** k) + rng.normal(0, 1.0, 2)
            w, h = max(w, 2.0), max(h, 2.0)
            if rng.random() < 0.02:
                h = 0.0                                             # degenerate detection
            bbox = np.around([cc[0] - w / 2, cc[1] - h / 2, cc[0] + w / 2, cc[1] + h / 2]).astype(np.int32)
            faces.append({'bbox': bbox, 'landmarks': np.zeros((5, 2), np.int32), 'score': np.float32(0.9)})
        if rng.random() < 0.15:                                     # a spurious one-frame detection
            x, y = rng.uniform(0, 1000, 2)
            faces.append({'bbox': np.array([x, y, x + 50, y + 60]).astype(np.int32),
                          'landmarks': np.zeros((5, 2), np.int32), 'score': np.float32(0.6)})
        order = rng.permutation(len(faces))
        faces = [faces[i] for i in order]
        for i, f in enumerate(faces):
            f['_i'] = i
        frames.append(faces)
    return frames


# ---- hand-built op programs: the GPU tests run them, tests/test_program_check_cpu.py holds each against the loader's program check ----
def conv_weights(L, rng):
    """Stem (3 -> c1, 3x3) and the conv under test (c1 -> cout, k x k, `groups`) of a layer dict."""
    c1, cout, k, groups = L['c1'], L['cout'], L['k'], L.get('groups', 1)
    W1 = rng.normal(0, 0.3, (c1, 3, 3, 3)).astype(np.float32)
    b1 = rng.normal(0, 0.1, c1).astype(np.float32)
    W2 = rng.normal(0, 1.0 / np.sqrt(c1 // groups * k * k), (cout, c1 // groups, k, k)).astype(np.float32)
    b2 = rng.normal(0, 0.1, cout).astype(np.float32)
    return W1, b1, W2, b2


def conv_case_program(L, variant, mid_f32, precision, split_io):
    """frames -> stem conv -> 'mid' -> the conv of layer dict `L` pinned to kernel `variant` (a lib.CONV_VARIANTS id) -> 'out'
    (+ 'res' / 'out2' where L asks).  -> (program, dict of the weights the reference needs)."""
    from terran_amd import pack
    rng = np.random.default_rng(11)
    c1, cout, k = L['c1'], L['cout'], L['k']
    stride, act = L.get('stride', 1), L.get('act', 0)
    W1, b1, W2, b2 = conv_weights(L, rng)
    P = pack.Program(pack.MODEL_OPENPOSE, precision)
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    t1 = P.tensor(c1, k // 2, name='mid', f32=mid_f32)
    P.conv(t0, t1, W1, b1, act=pack.ACT_RELU)
    t2 = P.tensor(L.get('out_total', cout), 0, name='out', f32=not split_io)
    kw = dict(variant=variant, groups=L.get('groups', 1))
    prelu = scale2 = shift2 = None
    if act == 2:
        prelu = rng.uniform(0.1, 0.4, cout).astype(np.float32)
        kw['prelu'] = prelu
    if L.get('res'):
        tres = P.tensor(cout, 0, name='res', f32=not split_io)
        Wr = rng.normal(0, 0.3, (cout, 3, 3, 3)).astype(np.float32)
        br = rng.normal(0, 0.1, cout).astype(np.float32)
        P.conv(t0, tres, Wr, br, stride=stride, pad=1)
        kw['res'] = tres
    if L.get('out2'):
        t3 = P.tensor(cout, 1, name='out2', f32=not split_io)
        scale2 = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        shift2 = rng.normal(0, 0.2, cout).astype(np.float32)
        kw.update(out2=t3, scale2=scale2, shift2=shift2)
    if L.get('pool'):
        kw['pool'] = True
    P.conv(t1, t2, W2, b2, stride=stride, act=act, out_ch_off=L.get('out_off', 0), cout_p=L.get('cout_p'), **kw)
    P.outputs = [t2]
    return P, dict(W2=W2, b2=b2, prelu=prelu, scale2=scale2, shift2=shift2)


def fc_program(variant, precision):
    """ArcFace's Flatten + Linear 25088 -> 512 as the 1x1 conv over the (N,1,1,25088) view of 'z'.  -> (program, Wl, bl)."""
    from terran_amd import pack
    rng = np.random.default_rng(12)
    P = pack.Program(pack.MODEL_OPENPOSE, precision)
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    Z = P.tensor(512, 0, name='z')
    W1 = rng.normal(0, 0.3, (512, 3, 3, 3)).astype(np.float32)
    b1 = rng.normal(0, 0.1, 512).astype(np.float32)
    P.conv(t0, Z, W1, b1, act=pack.ACT_RELU)
    A = P.tensor(7 * 7 * 512, 0, alias_of=Z)
    Wl = rng.normal(0, 1.0 / np.sqrt(25088), (512, 25088)).astype(np.float32)
    bl = rng.normal(0, 0.1, 512).astype(np.float32)
    f = np.arange(7 * 7 * 512)
    ch_pos = (f % 49) * 512 + f // 49                               # (C,H,W) flatten order -> NHWC position
    E = P.tensor(512, 0, name='emb', f32=True)
    P.conv(A, E, Wl.reshape(512, 25088, 1, 1), bl, ch_pos=ch_pos, pad=0, variant=variant)
    P.outputs = [E]
    return P, Wl, bl


def pinned_variant_program(variant):
    """One conv 3 -> 16 pinned to `variant`: Cin = 4, which only the table-driven kernel can run."""
    from terran_amd import pack
    rng = np.random.default_rng(1)
    P = pack.Program(pack.MODEL_OPENPOSE, 'f32')
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    t1 = P.tensor(16, 0, name='out')
    P.conv(t0, t1, rng.normal(0, 0.3, (16, 3, 3, 3)).astype(np.float32), np.zeros(16, np.float32), variant=variant)
    P.outputs = [t1]
    return P


def window_weights(L):
    """What every variant of a window-kernel layer shares (the rng goes on to draw each program's sink conv)."""
    rng = np.random.default_rng(23)
    W1, b1, W2, b2 = conv_weights(L, rng)
    cout = L['cout']
    prelu = rng.uniform(0.1, 0.4, cout).astype(np.float32)
    Wr, br = rng.normal(0, 0.3, (cout, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    return dict(rng=rng, W1=W1, b1=b1, W2=W2, b2=b2, prelu=prelu, Wr=Wr, br=br)


def window_program(L, variant, precision, wts):
    """frames -> stem -> 'mid' -> the conv of `L` pinned to `variant` -> 'out' (split format, halo 1) -> a float32 sink conv."""
    from terran_amd import pack
    c1, cout, k = L['c1'], L['cout'], L['k']
    P = pack.Program(pack.MODEL_OPENPOSE, precision)
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    t1 = P.tensor(c1, k // 2, name='mid')
    P.conv(t0, t1, wts['W1'], wts['b1'], act=pack.ACT_RELU)
    t2 = P.tensor(cout, 1, name='out')                       # split format (a conv reads it), halo 1
    kw = dict(variant=variant, groups=L.get('groups', 1), act=L.get('act', 0))
    if L.get('act') == 2:
        kw['prelu'] = wts['prelu']
    if L.get('res'):
        tres = P.tensor(cout, 0, name='res')
        P.conv(t0, tres, wts['Wr'], wts['br'], pad=1)
        kw['res'] = tres
    P.conv(t1, t2, wts['W2'], wts['b2'], **kw)
    t3 = P.tensor(32, 0, name='sink', f32=True)              # keeps `out` in the split format
    P.conv(t2, t3, wts['rng'].normal(0, 0.05, (32, cout, 3, 3)).astype(np.float32), np.zeros(32, np.float32))
    P.outputs = [t3]
    return P


def dwpw_block_program(C, cout, stride, split_out):
    """frames -> conv 3x3 (4 -> C, exact f32) -> [dw3x3 (stride) -> 1x1 C -> cout] (f16x3) [-> 1x1 conv (f16x3): the block's output is then
    stored pre-split] -> float32 out."""
    from terran_amd import pack
    rng = np.random.default_rng(1000 * C + 10 * cout + stride)
    P = pack.Program(pack.MODEL_OPENPOSE, 'f16x3')
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    P.input_stats = (np.array([-0.05] * 3 + [0.0]), np.array([0.08] * 3 + [0.0]))
    t1 = P.tensor(C, 1)
    P.conv(t0, t1, rng.normal(0, 0.3, (C, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, C).astype(np.float32), act=pack.ACT_RELU, precision='f32')
    t2 = P.tensor(cout, 0, name='block', f32=not split_out)
    P.dwpw(t1, t2, rng.normal(0, 0.3, (C, 1, 3, 3)).astype(np.float32), rng.normal(0, 0.1, C).astype(np.float32),
           rng.normal(0, 2.0 / np.sqrt(C), (cout, C, 1, 1)).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32),
           stride=stride, precision='f16x3')
    if split_out:
        t3 = P.tensor(32, 0, name='out', f32=True)
        P.conv(t2, t3, rng.normal(0, 0.05, (32, cout, 1, 1)).astype(np.float32), np.zeros(32, np.float32), precision='f16x3')
        P.outputs = [t3]
    else:
        P.outputs = [t2]
    return P


def lane_sharing_program():
    """Three convs, the middle one on lane 1: the last, on the main stream, reads what the lane wrote (the loader refuses that)."""
    from terran_amd import pack
    rng = np.random.default_rng(5)
    P = pack.Program(pack.MODEL_OPENPOSE, 'f32')
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    t1, t2, t3 = P.tensor(32, 1), P.tensor(32, 1), P.tensor(32, 0)
    w = lambda co, ci, k: rng.normal(0, 0.1, (co, ci, k, k)).astype(np.float32)
    P.conv(t0, t1, w(32, 3, 3), np.zeros(32, np.float32))
    P.lane = 1
    P.conv(t1, t2, w(32, 32, 3), np.zeros(32, np.float32))
    P.lane = 0
    P.conv(t2, t3, w(32, 32, 1), np.zeros(32, np.float32))          # reads the lane's output on the main stream
    P.outputs = [t3]
    return P


def two_conv_program(precision='f32', pad2=0, mid_halo=1, c=32, **second):
    """conv 4 -> c 3x3 pad 1 ('mid', halo `mid_halo`) into conv c -> c 3x3 pad `pad2` ('out', float32); `second`: further
    arguments of the second conv (groups, pool, k_split, ...)."""
    from terran_amd import pack
    rng = np.random.default_rng(8)
    P = pack.Program(pack.MODEL_OPENPOSE, precision)
    t0 = P.tensor(4, 1)
    P.input_tensor = t0
    t1 = P.tensor(c, mid_halo, name='mid')
    P.conv(t0, t1, rng.normal(0, 0.3, (c, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32), act=pack.ACT_RELU)
    t2 = P.tensor(c, 0, name='out', f32=True)
    P.conv(t1, t2, rng.normal(0, 0.1, (c, c, 3, 3)).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32), pad=pad2, **second)
    P.outputs = [t2]
    return P


# ---- the programs of tests/exact_programs.py on the GPU: bit equality with their float64 reference --------------------------------
def same(got, want, what):
    """Bit equality with float32(reference); the message names how many values differ and the first of them."""
    want = np.asarray(want).astype(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError('%s: %d of %d values differ, first at (n, c, y, x) = %s: got %r, want %r'
                             % (what, len(bad), got.size, i, float(got[i]), float(want[i])))


def run_exact(ctx, net, fr, names, what='', ref=None):
    """One forward of `net` on the frames `fr`; every tensor of `names` must equal the float64 reference (`ref`: one computed before
    for the same ops and frames).  -> the reference."""
    from terran_amd import lib
    from tests import exact_programs as ep
    m = getattr(net, 'model', None)
    if m is None:
        m = net.model = lib.Model(ctx, net.P)
    if ref is None:
        ref = ep.reference(net, fr)
    frames = ctx.upload(fr)
    m.forward_frames(frames)
    assert ctx.lib.ta_debug_range_check(ctx.h) == lib.OK, 'a tensor left the half-float range: the test program is wrong'
    for name in names:
        same(m.read(name), ref[name], '%s %s %s' % (what, fr.shape, name))
    frames.free()
    return ref


# ---- the detector's production entry, as RetinaFace._detect_arrays calls it -------------------------------------------------------
def retinaface_run(ctx, model, frames, threshold, nms_threshold, capacity, outputs=True):
    """One ta_retinaface_run on resident frames with room for `capacity` detections (outputs=False: null output pointers).
    -> (rc, counts (N,), boxes (capacity, 4), landmarks (capacity, 5, 2), scores (capacity,), required)."""
    import ctypes as C
    from terran_amd import lib
    counts = np.full(len(frames), -1, np.int32)
    boxes = np.full((max(capacity, 0), 4), np.nan, np.float32)
    lmks = np.full((max(capacity, 0), 5, 2), np.nan, np.float32)
    scores = np.full(max(capacity, 0), np.nan, np.float32)
    req = C.c_int32(-1)
    out = [lib.ptr(a) if outputs else None for a in (boxes, lmks, scores)]
    rc = ctx.lib.ta_retinaface_run(model.h, frames.h, float(threshold), float(nms_threshold), int(capacity), lib.ptr(counts),
                                   out[0], out[1], out[2], C.byref(req))
    return rc, counts, boxes, lmks, scores, int(req.value)
