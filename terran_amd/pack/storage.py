"""How a program's tensors are stored: the format of each (float32, pre-split bf16 / half-float pairs, plain half floats) and
the power of two each channel is stored times (module text of moments.py).  Both follow from the finished op list."""
import numpy as np

from .layout import FMT_F16, FMT_F32, OP_CONV, OP_COPYCH, OP_DWCONV, OP_DWPW, OP_MAXPOOL, OP_RFSTEM, SPLIT_FMT
from .moments import scale_exponents, spread_floor


def tensor_formats(P):
    """Storage format per tensor.  In the bf16 modes a tensor is kept PRE-SPLIT -- per pixel and 32-channel
    block, 32 bf16 `hi` then 32 bf16 `lo` (x = hi + lo; same 4 bytes per element as float32) -- when all of its
    conv consumers are whole-block reads by the pipelined kernel, whose MFMA operand fragments then come
    straight out of LDS with no conversion VALU.  Everything else stays float32."""
    # the arithmetic mode of a tensor's conv consumers decides its split format (a program may mix modes per op: the
    # detector's base runs exact f32, its refiner f16x3); consumers of different modes -> float32
    cprec = {}
    for op in P.ops:
        if op['type'] == OP_CONV:
            cprec.setdefault(op['in'], set()).add(op['prec'])
    fmt = []
    for t, (c, _, _) in enumerate(P.tensors):
        precs = cprec.get(t, {P.prec})
        p = next(iter(precs)) if len(precs) == 1 else 0
        fmt.append(SPLIT_FMT[p] if (P.allow_split and c % (64 if p == 4 else 32) == 0) else FMT_F32)
    for t in P.f32_only | {P.input_tensor}:
        fmt[t] = FMT_F32
    for op in P.ops:
        if op['type'] == OP_CONV:
            taps = op['kh'] * op['kw']
            pipe = (op['cin'] % 32 == 0 and op['in_ch_off'] % 32 == 0 and op['coutp'] % 64 == 0
                    and op['n_slabs'] >= 2 and op['n_slabs'] == taps * (op['cin'] // 32))
            if op['prec'] == 4:                          # half-float tensors: whole-tensor reads in slabs of 64 channels
                k64 = op['cin'] % 64 == 0 and op['n_slabs'] == taps * (op['cin'] // 64)      # already re-packed by blob()
                pipe = (pipe or (k64 and op['coutp'] % 64 == 0)) and \
                    op['cin'] % 64 == 0 and op['in_ch_off'] == 0 and op['groups'] == 1
            # the kernels that read pre-split tensors drain through LDS only: every channel slice of the op on an 8-channel
            # boundary (conv_igemm.hip: variant_eligible `staged`); anything else runs on the generic kernel, float32 in
            if op['out_ch_off'] % 8 or op['res_ch_off'] % 8 or op['out2_ch_off'] % 8:
                pipe = False
            if not pipe:
                fmt[op['in']] = FMT_F32
        elif op['type'] in (OP_DWPW, OP_RFSTEM):            # float32 in, float32 out
            fmt[op['in']] = FMT_F32
            if op['type'] == OP_RFSTEM:
                fmt[op['out']] = FMT_F32
        elif op['type'] == OP_COPYCH:
            if op['cin'] % 32 or op['in_ch_off'] % 32 or op['out_ch_off'] % 32:
                fmt[op['in']] = fmt[op['out']] = FMT_F32
        if op['type'] != OP_CONV:                       # half-float tensors are the conv kernels' alone
            for t in (op['in'], op['out']):
                if fmt[t] == FMT_F16:
                    fmt[t] = FMT_F32
    changed = True
    while changed:                                  # aliases share memory; copies are raw
        changed = False
        for t, (_, _, a) in enumerate(P.tensors):
            if a >= 0 and fmt[t] != fmt[a]:
                fmt[t] = fmt[a] = FMT_F32
                changed = True
        for op in P.ops:
            if op['type'] == OP_COPYCH and fmt[op['in']] != fmt[op['out']]:
                fmt[op['in']] = fmt[op['out']] = FMT_F32
                changed = True
    return fmt


def tensor_scales(P):
    """Exponents a[c] per tensor and channel: channel c is STORED times 2^a[c] (module text of moments.py).  All 0
    unless the program has half-float convs; 0 for the input, for tensors the host / post-processing kernels read
    unscaled (f32_only) and for anything a plain depthwise op touches.  Channels that are added (shortcuts), pooled,
    copied or seen through an alias share one exponent (union-find over (tensor, channel) nodes); a channel's exponent puts
    the largest bound of its group in (2^9, 2^10], but no channel sits more than 2^_CH_SPREAD below its tensor's largest."""
    n = len(P.tensors)
    sizes = [t[0] for t in P.tensors]
    scales = [np.zeros(c, np.int64) for c in sizes]
    if not P.scales_enabled or not any(op['type'] in (OP_CONV, OP_DWPW) and op['prec'] in (3, 4, 5) for op in P.ops):
        return scales
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    parent = np.arange(base[-1], dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union_run(ta, ca, tb, cb, cnt):
        for i in range(cnt):
            ra, rb = find(base[ta] + ca + i), find(base[tb] + cb + i)
            if ra != rb:
                parent[ra] = rb
    for t, (c, _, a) in enumerate(P.tensors):
        if a >= 0:
            ca = sizes[a]
            for p in range(c):
                ra, rb = find(base[t] + p), find(base[a] + p % ca)
                if ra != rb:
                    parent[ra] = rb
    fixed_t = set(P.f32_only) | {P.input_tensor}
    for op in P.ops:
        if op['type'] == OP_MAXPOOL:
            union_run(op['in'], 0, op['out'], 0, sizes[op['in']])
        elif op['type'] == OP_COPYCH:
            union_run(op['in'], op['in_ch_off'], op['out'], op['out_ch_off'], op['cin'])
        elif op['type'] == OP_DWCONV:
            fixed_t |= {op['in'], op['out']}
        elif op['type'] == OP_CONV and op['res'] >= 0:
            union_run(op['res'], op['res_ch_off'], op['out'], op['out_ch_off'], op['cout'])
    amax = np.concatenate([P.expected_amax(t, per_channel=True) for t in range(n)])
    # no channel more than 2^_CH_SPREAD below its tensor's largest: a channel's own bound is a noisier number than the tensor's
    # (a mis-predicted weak channel must not be blown up into the end of the range), and 2^8 of relief already keeps a
    # channel 2^14 below the tensor's largest inside the window where hi + lo carries all its bits
    for t in range(n):
        seg = amax[base[t]:base[t + 1]]
        if len(seg) and seg.max() > 0:
            np.maximum(seg, np.where(seg > 0, spread_floor(seg.max()), 0.0), out=seg)
    roots = np.array([find(i) for i in range(base[-1])], np.int64)
    gmax = np.zeros(base[-1])
    np.maximum.at(gmax, roots, amax)
    fixed = np.zeros(base[-1], bool)
    for t in fixed_t:
        fixed[roots[base[t]:base[t + 1]]] = True
    forced = {}
    for t, e in P.forced_scale.items():
        if isinstance(t, (int, np.integer)):
            for r in roots[base[t]:base[t + 1]]:
                forced[int(r)] = int(e)
    g = gmax[roots]
    ok = np.isfinite(g) & (g > 0) & ~fixed[roots]
    expo = np.zeros(base[-1], np.int64)
    expo[ok] = scale_exponents(g[ok])
    for r, e in forced.items():
        if not fixed[r]:
            expo[roots == r] = e
    return [expo[base[t]:base[t + 1]].copy() for t in range(n)]
