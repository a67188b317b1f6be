"""`Program`: the tensors, ops and weight region of one model, and the blob they become.

The emitters (`conv`, `dwconv`, `rfstem`, `dwpw`, `simple`) record an op, its weights and the moments of what it writes; `blob()`
then settles every tensor's storage format and activation exponents and folds the powers of two into the weights and epilogue
vectors each op type keeps (`_finish_conv`, `_finish_dwpw`, `_finish_rfstem`)."""
import json
import os

import numpy as np

from . import moments, storage
from .layout import (ACT_NONE, ACT_RELU, BLOB_VERSION, FMT_F16, HEADER_DT, MAGIC, OP_CONV, OP_DT, OP_DWCONV, OP_DWPW, OP_MAXPOOL,
                     OP_RFSTEM, PRECISIONS, TENSOR_DT, WeightRegion, _rup, fold_input_affine, op_desc, pack_rows)
from .moments import ChannelStats, act_bound, act_moments


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e).astype(np.int32))


class Program:
    """Accumulates tensors, ops and the weight region of one model."""

    def __init__(self, kind, precision='f32'):
        self.kind = kind
        self.precision = precision
        self.prec = PRECISIONS[precision]
        self.tensors = []      # (channels, halo, alias_of)
        self.ops = []
        self.w = WeightRegion()
        self.names = {}        # debug taps: name -> (tensor, ch_off, ch)
        self.extra = {}        # JSON-able notes that travel with the repack cache (save_cache / from_cache)
        self.input_tensor = None
        self.outputs = []
        self.f32_only = set()
        self.allow_split = True
        self.lane = 0          # convs emitted while this is 1 / 2 run on that side stream (ta_op_desc.variant bits 17..18)
        # activation scales (module text of moments.py): per tensor and channel the expected (mean, variance) of what the
        # ops write, in program order; `_fold[op]` keeps the un-scaled epilogue vectors until blob() knows every tensor's scale
        self.stats = {}        # tensor -> ChannelStats
        self._fold = {}
        self.input_stats = None                # (mean, var) per input channel; default N(0, 1)
        self.forced_scale = {}                 # tensor (or ('mid', op index): a dw+pw block's depthwise intermediate) -> exponent
                                               # (tests: provoke / avoid the half-float range)
        self.scales_enabled = not os.environ.get('TERRAN_AMD_NO_ACT_SCALES')     # A/B switch: every tensor stored unscaled

    def tensor(self, channels, halo, alias_of=-1, name=None, f32=False):
        """f32=True pins the tensor to plain float32 (outputs read by post-processing kernels / the host).
        alias_of=-2: shape only, never materialised (the input of a program whose first op reads the frames itself)."""
        assert channels % 4 == 0
        self.tensors.append((channels, halo, alias_of))
        tid = len(self.tensors) - 1
        if f32:
            self.f32_only.add(tid)
        if name:
            self.names[name] = (tid, 0, channels)
        return tid

    def tap(self, name, tid, ch_off, ch):
        self.names[name] = (tid, ch_off, ch)

    def _stats_of(self, tid):
        """Expected moments per channel of tensor `tid`; an alias gets a copy of its target's (what is written to it is lost)."""
        c, _, a = self.tensors[tid]
        if a >= 0:                                    # (N,1,1,H*W*C) view of tensor `a`: position-major, channel fastest
            st = self._stats_of(a)
            return st.tiled(c // len(st.mean))
        if tid not in self.stats:
            mu, var = np.zeros(c), np.ones(c)
            if tid == self.input_tensor and self.input_stats is not None:
                m_, v_ = self.input_stats
                mu[:len(m_)], var[:len(v_)] = m_, v_
            self.stats[tid] = ChannelStats.unwritten(mu, var)
            if tid == self.input_tensor:
                self.stats[tid].written[:] = True
        return self.stats[tid]

    def _emit(self, op, fold=None):
        if fold is not None:
            self._fold[len(self.ops)] = fold
        self.ops.append(op)

    # ---- op emitters ---------------------------------------------------------------------------------------------------
    def conv(self, tin, tout, W, bias, *, stride=1, pad=None, act=ACT_NONE, in_ch_off=0, ch_pos=None, cin_p=None,
             out_ch_off=0, cout_p=None, prelu=None, res=-1, res_ch_off=0, res_up2=0, out2=-1, out2_ch_off=0,
             scale2=None, shift2=None, groups=1, variant=0, pool=False, k_split=0, precision=None, in_affine=None):
        """W: (cout, cin, kh, kw) float (BN already folded), bias: (cout,).
        ch_pos[ci] = position of true input channel ci inside the slice [in_ch_off, in_ch_off+cin_p).
        groups > 1: W is (cout, cin / groups, kh, kw) as in torch; group g reads input channels
        [in_ch_off + g cin_g, + cin_g) and writes output channels [out_ch_off + g cout_g, + cout_g); cin_g a multiple
        of 32 and cout_g of 128 (a 128-channel output tile never straddles two groups).
        variant != 0 pins the conv to one kernel variant (lib.CONV_VARIANTS; parity tests): loading fails when that
        kernel cannot run the layer.
        in_affine=(scale, shift) per input channel: the conv computes conv(pad0(scale * x + shift)) -- ArcFace's BatchNorm in
        front of a zero-padded conv (arcface/model.py:12-14) -- with the scale folded into the weights and the shift into
        one bias per border class of the output pixel (nine on ordinary maps) (the shift reaches the sum only through taps that are not padding;
        3x3, stride 1, pad 1 only).  The input tensor is then read raw: no BatchNorm'd copy of it has to exist.
        k_split > 1: the layer's K is cut in that many fixed ranges (one workgroup each, ordered reduction): for layers whose
        output is too small to fill the chip at any batch in use.  A property of the LAYER, never of the batch.
        pool=True fuses the 2x2 / 2 max-pool that follows the conv (+ activation) into its epilogue: `tout` is the POOLED
        tensor (split-role kernel only: cin % 32 == 0, cout % 64 == 0, plain epilogue)."""
        W = np.asarray(W, dtype=np.float64)
        cout, cin, kh, kw = W.shape
        bias9 = None
        if in_affine is not None:
            assert (kh, kw, stride) == (3, 3, 1) and pad in (None, 1) and groups == 1 and out2 < 0 and scale2 is None and not pool
            W, bias9 = fold_input_affine(W, bias, *in_affine)
            bias = bias9[5]                                               # (middle, middle): the interior
        if groups > 1:
            assert cout % groups == 0 and cin % 32 == 0 and (cout // groups) % 128 == 0 and ch_pos is None
        if pad is None:
            pad = kh // 2
        if pool:
            assert groups == 1 and res < 0 and out2 < 0 and stride == 1 and cin % 32 == 0 and cout % 64 == 0 and ch_pos is None
        if cin_p is None:
            cin_p = _rup(cin, 4)
        if ch_pos is None:
            ch_pos = np.arange(cin)
        if cout_p is None:
            cout_p = _rup(cout, 4)
        coutp = _rup(cout_p, 32)
        K = kh * kw * cin_p
        n_slabs = _rup(K, 32) // 32
        full = np.zeros((kh * kw, cin_p, coutp), np.float32)
        full[:, np.asarray(ch_pos), :cout] = W.transpose(2, 3, 1, 0).reshape(kh * kw, cin, cout)
        flat = np.zeros((n_slabs * 32, coutp), np.float32)
        flat[:K] = full.reshape(K, coutp)
        prec = self.prec if precision is None else PRECISIONS[precision]      # a single op may run in another arithmetic mode
        # the weights are packed by blob(): their columns absorb the input channels' activation exponents first

        def vec(v, fill=0.0):
            if v is None:
                return -1, None
            out = np.full(coutp, fill, np.float64)
            out[:cout] = np.asarray(v, dtype=np.float64)
            return self.w.add(out), out
        fold = dict(flat=flat, taps=kh * kw, cin_p=cin_p, K=K)
        if bias9 is not None:                                             # [16][coutp] in the place of the (absent) second output's scale
            t9 = np.zeros((16, coutp), np.float64)
            t9[:, :cout] = bias9
            scale2_off = self.w.add(t9)
            fold['bias9'] = t9
            variant |= 1 << 16
        else:
            scale2_off, fold['scale2'] = vec(scale2)
        bvec = np.zeros(coutp, np.float64)
        if bias is not None:
            bvec[:cout] = np.asarray(bias, np.float64)
        fold['bias'] = bvec
        bias_off = self.w.add(np.concatenate([bvec, np.ones(coutp)]))    # [bias | per-channel un-scale]: one pointer for the kernels
        prelu_off, _ = vec(prelu)
        shift2_off, fold['shift2'] = vec(shift2)
        self._emit(op_desc(OP_CONV, tin, tout, cin_p, cout_p, in_ch_off=in_ch_off, out_ch_off=out_ch_off, coutp=coutp, kh=kh, kw=kw,
                           stride=stride, pad=pad, act=act, res=res, res_ch_off=res_ch_off, res_up2=res_up2, out2=out2,
                           out2_ch_off=out2_ch_off, n_slabs=n_slabs, prec=prec, groups=groups,
                           variant=variant | (int(k_split) << 8) | (self.lane << 17), pool=int(bool(pool)),
                           w_off=self.w.reserve(n_slabs * coutp * 128), bias_off=bias_off, prelu_off=prelu_off,
                           scale2_off=scale2_off, shift2_off=shift2_off, wus_off=bias_off + 4 * coutp,
                           macs_per_pixel=float(cout * cin * kh * kw)), fold)
        # ---- expected moments of what this op writes
        st_in = self._stats_of(tin)
        span = slice(in_ch_off, in_ch_off + cin_p * max(groups, 1))
        mu, var = moments.conv_moments(full, bias, st_in.mean[span], st_in.var[span], groups, cout)
        slope = None if prelu is None else np.asarray(prelu, np.float64)
        bound = act_bound(mu, var, act, slope)
        mu, var = act_moments(mu, var, act, slope)
        if res >= 0:
            st_r, rs = self._stats_of(res), slice(res_ch_off, res_ch_off + cout)
            mu, var, bound = mu + st_r.mean[rs], var + st_r.var[rs], bound + st_r.amax[rs]
        if pool:
            mu, var = moments.pool_moments(mu, var)
        self._stats_of(tout).write(out_ch_off, mu, var, bound)
        if out2 >= 0:
            s2, h2 = np.asarray(scale2, np.float64), np.asarray(shift2, np.float64)
            self._stats_of(out2).write(out2_ch_off, mu * s2 + h2, var * s2 * s2, np.abs(s2) * bound + np.abs(h2))

    def dwconv(self, tin, tout, W, bias, *, stride=1, relu=True):
        """W: (C,1,3,3) folded, bias (C,).  (The layer-by-layer detector program: float32 tensors, stored unscaled.)"""
        C = W.shape[0]
        w9 = np.asarray(W, dtype=np.float64).reshape(C, 9).T            # [9][C]
        act = ACT_RELU if relu else ACT_NONE
        self._emit(op_desc(OP_DWCONV, tin, tout, C, C, coutp=_rup(C, 32), kh=3, kw=3, stride=stride, pad=1, act=act,
                           w_off=self.w.add(w9), bias_off=self.w.add(bias), macs_per_pixel=float(C * 9)))
        st = self._stats_of(tin)
        mu, var = moments.dw_moments(w9, bias, st.mean[:C], st.var[:C])
        self._stats_of(tout).write(0, *act_moments(mu, var, act), act_bound(mu, var, act))

    def rfstem(self, tin, tout, Ws, bs, Wd, bd, Wp, bp, Wd2=None, bd2=None, Wp2=None, bp2=None):
        """RetinaFace front as ONE op: conv3x3 s2 (3 -> 8) -> depthwise 3x3 (8) -> 1x1 (8 -> 16), each + folded BN + ReLU.
        Ws (8,3,3,3) / bs (8,), Wd (8,1,3,3) / bd (8,), Wp (16,8,1,1) / bp (16,), all already folded.
        With Wd2 (16,1,3,3) / bd2 (16,), Wp2 (32,16,1,1) / bp2 (32,): the NEXT block of the base -- depthwise 3x3 stride 2 (16) ->
        1x1 (16 -> 32), retinaface/model.py:26-39 -- in the same kernel: `tout` is the 32-channel quarter-resolution map and
        the 16-channel half-resolution map (the largest tensor of the network) never reaches HBM."""
        parts = [np.asarray(Ws, np.float64).reshape(8, 27).ravel(), np.asarray(bs, np.float64),
                 np.asarray(Wd, np.float64).reshape(8, 9).T.ravel(), np.asarray(bd, np.float64),
                 np.asarray(Wp, np.float64).reshape(16, 8).ravel(), np.asarray(bp, np.float64)]
        blocks = [(Wd, bd, Wp, bp)]
        fuse = Wd2 is not None
        if fuse:                        # [9][16] depthwise taps, [16] bias, [16][32] 1x1 as (c, oc), [32] bias: what rf_stem_kernel<true> reads
            parts += [np.asarray(Wd2, np.float64).reshape(16, 9).T.ravel(), np.asarray(bd2, np.float64),
                      np.asarray(Wp2, np.float64).reshape(32, 16).T.ravel(), np.asarray(bp2, np.float64)]
            blocks.append((Wd2, bd2, Wp2, bp2))
        blob = np.concatenate(parts)
        assert blob.size == (448 + 704 if fuse else 448)
        self._emit(op_desc(OP_RFSTEM, tin, tout, 4, 32 if fuse else 16, coutp=32, kh=3, kw=3, stride=2, pad=1, act=ACT_RELU,
                           w_off=self.w.add(blob), macs_per_pixel=float(8 * 27 + 16 * 8) + (32 * 16 / 4.0 if fuse else 0.0)),
                   dict(rfstem=parts))
        # moments: the frames are raw 0..255 BGR pixels (the kernel reads them itself: no float copy exists)
        st = self._stats_of(tin)
        mu, var = moments.rfstem_moments(st.mean[:3], st.var[:3], Ws, bs, blocks)
        self._stats_of(tout).write(0, *act_moments(mu, var, ACT_RELU), act_bound(mu, var, ACT_RELU))

    def dwpw(self, tin, tout, Wd, bd, Wp, bp, *, stride=1, precision=None):
        """Depthwise 3x3 (stride 1 / 2, pad 1) + ReLU fused into the following 1x1 conv + ReLU (both BN-folded):
        Wd (C,1,3,3) / bd (C,), Wp (cout, C, 1, 1) / bp (cout,).  The depthwise part is float32 FMAs; the 1x1 runs on the
        exact-f32 MFMA or (precision='f16x3') on the split-half MFMA."""
        prec = self.prec if precision is None else PRECISIONS[precision]
        assert prec in (0, 3), 'the fused depthwise + pointwise block exists in the f32 and f16x3 modes'
        C = Wd.shape[0]
        Wp = np.asarray(Wp, np.float64)
        cout = Wp.shape[0]
        assert Wp.shape[1] == C and C % 4 == 0 and cout % 4 == 0
        coutp = _rup(cout, 32)
        n_slabs = _rup(C, 32) // 32
        flat = np.zeros((n_slabs * 32, coutp), np.float32)
        flat[:C, :cout] = Wp.reshape(cout, C).T
        bias = np.zeros(coutp, np.float64)
        bias[:cout] = np.asarray(bp, np.float64)
        w9 = np.asarray(Wd, np.float64).reshape(C, 9).T                                          # [9][C]
        bd = np.asarray(bd, np.float64)
        # moments: depthwise (+ ReLU) -> the intermediate that is split into half floats in registers -> 1x1 (+ ReLU)
        st = self._stats_of(tin)
        mu0, var0 = moments.dw_moments(w9, bd, st.mean[:C], st.var[:C])
        mid_bound = act_bound(mu0, var0, ACT_RELU)                        # per channel: the depthwise result is per channel
        w_off = self.w.reserve(n_slabs * coutp * 128)
        bias_off = self.w.add(np.concatenate([bias, np.ones(coutp)]))    # [bias | per-channel un-scale], as for a conv
        self._emit(op_desc(OP_DWPW, tin, tout, C, cout, coutp=coutp, stride=stride, act=ACT_RELU, n_slabs=n_slabs, prec=prec,
                           w_off=w_off, bias_off=bias_off, scale2_off=self.w.add(w9), shift2_off=self.w.add(bd),
                           wus_off=bias_off + 4 * coutp, macs_per_pixel=float(cout * C)),
                   dict(flat=flat, bias=bias, dw_w=w9, dw_b=bd, mid_bound=mid_bound))
        mu2, var2 = moments.pointwise_moments(Wp.reshape(cout, C), bias[:cout], *act_moments(mu0, var0, ACT_RELU))
        self._stats_of(tout).write(0, *act_moments(mu2, var2, ACT_RELU), act_bound(mu2, var2, ACT_RELU))

    def simple(self, typ, tin, tout, in_ch_off=0, out_ch_off=0, ch=0):
        """OP_MAXPOOL (2x2 / 2, whole tensor) or OP_COPYCH (`ch` channels from one slice to another)."""
        self._emit(op_desc(typ, tin, tout, ch, ch, in_ch_off=in_ch_off, out_ch_off=out_ch_off, kh=2, kw=2, stride=2))
        st = self._stats_of(tin)
        if typ == OP_MAXPOOL:
            self._stats_of(tout).write(0, *moments.pool_moments(st.mean, st.var), st.amax.copy())
        else:
            sl = slice(in_ch_off, in_ch_off + ch)
            self._stats_of(tout).write(out_ch_off, st.mean[sl].copy(), st.var[sl].copy(), st.amax[sl].copy())

    # ---- the repack cache file -------------------------------------------------------------------------------------------
    @classmethod
    def from_cache(cls, path):
        """Load a program written by `save_cache` (packed blob + debug-tap names)."""
        with open(path, 'rb') as f:
            head = f.read(16)
            if head[:8] != b'TAMCACHE':
                raise ValueError('not a pack cache file')
            n = int.from_bytes(head[8:16], 'little')
            meta = json.loads(f.read(n).decode())
            blob = f.read()
        self = cls(meta['kind'], meta['precision'])
        self.names = {k: tuple(v) for k, v in meta['names'].items()}
        self.outputs = meta['outputs']
        self.extra = dict(meta.get('extra') or {})
        self._blob = blob
        return self

    def save_cache(self, path):
        # `extra`: decisions taken about this program after packing (arcface.guard_f16x2's calibration result) -- kept with the blob
        meta = json.dumps({'kind': self.kind, 'precision': self.precision, 'names': self.names,
                           'outputs': [int(o) for o in self.outputs], 'extra': getattr(self, 'extra', {})}).encode()
        tmp = path + '.tmp.%d' % os.getpid()
        with open(tmp, 'wb') as f:
            f.write(b'TAMCACHE' + len(meta).to_bytes(8, 'little') + meta + self.blob())
        os.replace(tmp, path)                      # atomic: concurrent ranks may race to write the same file

    # ---- storage formats and activation exponents ------------------------------------------------------------------------
    def tensor_formats(self):
        """Storage format per tensor (storage.tensor_formats)."""
        return storage.tensor_formats(self)

    def expected_amax(self, tid, per_channel=False):
        """Largest |x| the packer expects in tensor `tid` (per channel: the bound of every channel some op writes, else 0)."""
        st = self._stats_of(tid)
        am = np.where(st.written, st.amax, 0.0)
        return am if per_channel else float(am.max()) if len(am) else 0.0

    def tensor_scales(self):
        """Exponents a[c] per tensor and channel: channel c is STORED times 2^a[c] (storage.tensor_scales)."""
        return storage.tensor_scales(self)

    # ---- the blob --------------------------------------------------------------------------------------------------------
    def blob(self):
        if getattr(self, '_blob', None) is not None:
            return self._blob
        fmts = self.tensor_formats()
        self.scales = scales = self.tensor_scales()
        tens = self._tensor_table(fmts, scales)
        # epilogue vectors with every power of two folded in: the sums of channel co arrive times 2^s[co] (the activation
        # exponents of the input channels are inside the weights), the results leave times 2^a_out[co]
        self.mid_scales = {}
        finish = {OP_CONV: self._finish_conv, OP_DWPW: self._finish_dwpw, OP_RFSTEM: self._finish_rfstem}
        for i, f in self._fold.items():
            op = self.ops[i]
            finish[op['type']](i, op, f, scales[op['in']], self._exponents(scales, op, 'out'), fmts)
        ops = np.zeros(len(self.ops), OP_DT)
        for i, op in enumerate(self.ops):
            for k, v in op.items():
                ops[i][k] = v
        t_off = HEADER_DT.itemsize
        o_off = t_off + tens.nbytes
        w_off = _rup(o_off + ops.nbytes, 256)
        outs = np.full(16, -1, np.int32)
        outs[:len(self.outputs)] = self.outputs
        hdr = np.zeros(1, HEADER_DT)
        hdr[0] = (MAGIC, BLOB_VERSION, self.kind, len(self.tensors), len(self.ops), self.input_tensor, len(self.outputs), outs,
                  t_off, o_off, w_off, self.w.nbytes)
        head = hdr.tobytes() + tens.tobytes() + ops.tobytes()
        for f in self._fold.values():                 # the float32 weight matrices are not needed any more
            f.pop('flat', None)
        self._blob = head + b'\0' * (w_off - len(head)) + self.w.tobytes()     # a program is packed once
        return self._blob

    def _tensor_table(self, fmts, scales):
        """ta_tensor_desc per tensor.  One with a non-zero exponent anywhere gets [C] floats 2^-a[c] in the weights region (debug
        taps and the pose post-processing multiply what they read with it)."""
        tens = np.zeros(len(self.tensors), TENSOR_DT)
        for i, (c, h, a) in enumerate(self.tensors):
            unscale_off = self.w.add(_pow2(-scales[i])) if np.any(scales[i] != 0) else -1
            assert unscale_off < 2 ** 31
            tens[i] = (c, h, a, fmts[i], unscale_off)
        return tens

    @staticmethod
    def _exponents(scales, op, which):
        """The exponents of the channel slice op[which] (`out` / `out2`) writes, padded with 0 to coutp."""
        a = np.zeros(op['coutp'], np.int64)
        off = op[which + '_ch_off']
        seg = scales[op[which]][off:off + op['cout']]
        a[:len(seg)] = seg
        return a

    def _rewrite_bias(self, op, f, a_out, wexp):
        """[bias 2^a_out | un-scale 2^(a_out - wexp)]: the sums arrive times the weight rows' 2^wexp, the results leave times 2^a_out."""
        self.w.rewrite(op['bias_off'], np.concatenate([f['bias'] * _pow2(a_out), _pow2(a_out - wexp)]))

    @staticmethod
    def _fold_input_exponents(op, f, a_in):
        """The (n_slabs * 32, coutp) weights of conv `op` with 2^-a_in[c] folded into the rows of input channel c (exact)."""
        flat, taps, cin_p, K = f['flat'], f['taps'], f['cin_p'], f['K']
        groups = max(op['groups'], 1)
        cols = a_in[op['in_ch_off']:op['in_ch_off'] + cin_p * groups]
        if not np.any(cols != 0):
            return flat
        fs = flat.copy()
        cg = op['cout'] // groups if groups > 1 else flat.shape[1]      # group g: its own input channels, its own output columns
        for g in range(groups):
            e = -np.tile(cols[g * cin_p:(g + 1) * cin_p], taps).astype(np.int32)
            fs[:K, g * cg:(g + 1) * cg] = np.ldexp(flat[:K, g * cg:(g + 1) * cg], e[:, None])
        return fs

    def _finish_conv(self, i, op, f, a_in, a_out, fmts):
        fs = self._fold_input_exponents(op, f, a_in)
        data, wexp = pack_rows(fs, op['coutp'], op['prec'])
        # 'f16' mode: a conv whose input tensor is stored as plain half floats (TA_FMT_F16) walks K in slabs of 64
        # channels -- a slab row is 64 halfs of ONE operand, not [hi x32 | lo x32] -- half the bytes of the image reserved
        if op['prec'] == 4 and fmts[op['in']] == FMT_F16:
            cin_p, K, coutp = f['cin_p'], f['K'], op['coutp']
            assert cin_p % 64 == 0 and op['in_ch_off'] == 0 and op['groups'] == 1
            rows = np.ldexp(fs[:K].reshape(K // 64, 64, coutp).transpose(0, 2, 1), wexp[None, :, None].astype(np.int32)).astype(np.float16)   # [slab][cout][64]
            assert rows.nbytes * 2 == len(data)
            data = rows.tobytes() + b'\0' * rows.nbytes
            op['n_slabs'] = K // 64
            f['rows64'] = rows
        f['wexp'] = wexp
        self.w.rewrite(op['w_off'], data)
        self._rewrite_bias(op, f, a_out, wexp)
        if 'bias9' in f:
            self.w.rewrite(op['scale2_off'], f['bias9'] * _pow2(a_out)[None, :])
        elif op['out2'] >= 0:
            a2 = self._exponents(self.scales, op, 'out2')
            self.w.rewrite(op['scale2_off'], f['scale2'] * _pow2(a2 - a_out))
            self.w.rewrite(op['shift2_off'], f['shift2'] * _pow2(a2))

    def _finish_dwpw(self, i, op, f, a_in, a_out, fmts):
        # the depthwise result is split into half floats in registers (f16x3): per channel an exponent of its own
        C = op['cin']
        a_mid = np.zeros(C, np.int64)
        if op['prec'] == 3 and self.scales_enabled:
            mb = f['mid_bound']
            okc = np.isfinite(mb) & (mb > 0)
            if okc.any():
                a_mid[okc] = moments.scale_exponents(np.maximum(mb, moments.spread_floor(mb[okc].max()))[okc])
        elif op['prec'] == 0:
            a_mid = a_in[:C].copy()                             # exact f32: any power of two gives the same bits
        if ('mid', i) in self.forced_scale:
            a_mid[:] = int(self.forced_scale[('mid', i)])
        self.mid_scales[i] = a_mid
        self.w.rewrite(op['scale2_off'], f['dw_w'] * _pow2(a_mid - a_in[:C])[None, :])
        self.w.rewrite(op['shift2_off'], f['dw_b'] * _pow2(a_mid))
        fl = f['flat'].copy()
        fl[:C] = np.ldexp(fl[:C], -a_mid.astype(np.int32)[:, None])
        data, wexp = pack_rows(fl, op['coutp'], op['prec'])
        self.w.rewrite(op['w_off'], data)
        self._rewrite_bias(op, f, a_out, wexp)

    def _finish_rfstem(self, i, op, f, a_in, a_out, fmts):
        parts, up = list(f['rfstem']), _pow2(a_out)
        if len(parts) == 10:        # fused second block: the stored tensor is ITS output; the 16-channel map stays inside the kernel
            parts[8] = (parts[8].reshape(16, 32) * up[None, :32]).ravel()
            parts[9] = parts[9] * up[:32]
        else:
            parts[4] = (parts[4].reshape(16, 8) * up[:16, None]).ravel()
            parts[5] = parts[5] * up[:16]
        self.w.rewrite(op['w_off'], np.concatenate(parts))
