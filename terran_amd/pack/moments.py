"""Moment propagation: the plan-time activation scales of the half-float modes.

The switches of the scale assignment (_ACT_TARGET_LOG2, _CH_SPREAD) are read here and nowhere else: an experiment that varies
them assigns them on THIS module."""
from dataclasses import dataclass

import numpy as np

from .layout import ACT_NONE, ACT_RELU

# The half-float formats of the f16x3 / f16 modes keep all their bits for |x| in [2^-3, 65504] only (TA_FMT_SPLIT16:
# the lo half goes subnormal below; TA_FMT_F16: 2^-14).  Every CHANNEL of every tensor of a program with half-float convs is
# therefore STORED times a power of two 2^a[c] chosen at pack time so that the channel's largest expected |x| 2^a[c] lands
# near 2^10 -- 64 x of headroom to the end of the range, 13 binades of full precision below -- whatever the other channels
# of the tensor do (trained networks spread their channels over orders of magnitude).  It costs the kernels nothing: a
# consumer's weights absorb 2^-a[c] per INPUT channel (exact: powers of two, before the hi | lo split), a producer's
# per-channel epilogue vectors absorb 2^a[co] (bias, un-scale; ReLU and PReLU are positively homogeneous), tensors that are
# added (shortcuts), pooled, copied or aliased share their exponents.  The expectation comes from propagating per-channel
# (mean, variance) through the folded weights: Gaussian moments through ReLU / PReLU, independent channels, half-correlated
# filter taps.  It only has to be right to within a few binades: a channel that still overflows raises the range flag
# (TA_E_RANGE -> the wrappers' exact-f32 re-run).
_SQRT2, _SQRT2PI = np.sqrt(2.0), np.sqrt(2.0 * np.pi)
_TAP_CORR = 0.5          # share of the variance that adds coherently over the taps of a k x k filter (smooth images)
_ACT_TARGET_LOG2 = 10    # estimated max |x| 2^a in (2^9, 2^10]
_ACT_SIGMAS = 6.0
_CH_SPREAD = 8           # channel exponents of one tensor differ by at most this much


def default_bound(mu, var):
    return np.abs(mu) + _ACT_SIGMAS * np.sqrt(var)


def scale_exponents(bound):
    """Exponents a that put `bound` 2^a in (2^(_ACT_TARGET_LOG2 - 1), 2^_ACT_TARGET_LOG2]; bound finite and > 0."""
    return np.clip(_ACT_TARGET_LOG2 - np.ceil(np.log2(bound)), -40, 40).astype(np.int64)


def spread_floor(top):
    """The least bound a channel is scaled for when the largest of its tensor is `top`."""
    return top * 2.0 ** -_CH_SPREAD


@dataclass
class ChannelStats:
    """What the ops are expected to write into a tensor, per channel, in program order."""
    mean: np.ndarray
    var: np.ndarray
    written: np.ndarray       # bool: some op writes the channel
    amax: np.ndarray          # bound on |x| the channel is expected to reach

    @classmethod
    def unwritten(cls, mean, var):
        return cls(mean, var, np.zeros(len(mean), bool), default_bound(mean, var))

    def tiled(self, rep):
        return ChannelStats(np.tile(self.mean, rep), np.tile(self.var, rep), np.tile(self.written, rep), np.tile(self.amax, rep))

    def write(self, ch_off, mu, var, amax=None):
        """amax: bound on |x| per channel (default |mean| + 6 sigma); a rectified channel passes the bound of its positive tail,
        NOT the moments of the rectified variable -- a channel that is almost always zero still reaches that tail somewhere
        in a batch of 10^7 pixels."""
        sl = slice(ch_off, ch_off + len(mu))
        if amax is None:
            amax = default_bound(mu, var)
        new = ~self.written[sl]
        # a slice written by several ops (ping-pong stage tensors): moments of the writer with the larger bound, largest bound
        take = new | (amax > self.amax[sl])
        self.mean[sl][take] = mu[take]
        self.var[sl][take] = var[take]
        self.amax[sl] = np.where(new, amax, np.maximum(amax, self.amax[sl]))
        self.written[sl] = True


def _erf(x):
    from math import erf
    return np.vectorize(erf, otypes=[np.float64])(x)


def act_moments(mu, var, act, slope=None):
    """(mean, variance) of relu(z) / prelu(z, slope) for z ~ N(mu, var), element-wise."""
    if act == ACT_NONE:
        return mu, var
    mu, var = np.asarray(mu, np.float64), np.maximum(np.asarray(var, np.float64), 1e-60)
    sd = np.sqrt(var)
    t = mu / sd
    Phi = 0.5 * (1.0 + _erf(t / _SQRT2))
    phi = np.exp(-0.5 * t * t) / _SQRT2PI
    m_pos = mu * Phi + sd * phi
    s_pos = (mu * mu + var) * Phi + mu * sd * phi
    m_neg = -mu * (1.0 - Phi) + sd * phi
    s_neg = (mu * mu + var) * (1.0 - Phi) - mu * sd * phi
    a = np.zeros_like(mu) if (act == ACT_RELU or slope is None) else np.asarray(slope, np.float64)
    m = m_pos - a * m_neg
    s2 = s_pos + a * a * s_neg
    return m, np.maximum(s2 - m * m, 0.0)


def act_bound(mu, var, act, slope=None):
    """Bound on |act(z)| for z ~ N(mu, var): the 6-sigma tails of z pushed through the activation."""
    sd = np.sqrt(np.maximum(var, 0.0))
    hi, lo = mu + _ACT_SIGMAS * sd, _ACT_SIGMAS * sd - mu            # reach of the positive / negative tail
    if act == ACT_NONE:
        return np.maximum(hi, lo)
    # a channel the moments call (almost) always off may still fire: the mean of a deep channel is the least certain number
    # here, so a rectified channel is never given less than 4 sigma of reach
    if act == ACT_RELU or slope is None:
        return np.maximum(hi, 4.0 * sd)
    a = np.abs(np.asarray(slope, np.float64))
    return np.maximum(np.maximum(hi, a * lo), 4.0 * sd * np.maximum(a, 1.0))


def conv_moments(full, bias, mu_in, var_in, groups, cout):
    """full: (taps, cin_p, coutp) weights at their physical input positions; -> (mean, var) of the `cout` sums."""
    taps, cin_p, coutp = full.shape
    f64 = full.astype(np.float64)
    wsum = f64.sum(0)                                          # (cin_p, coutp)
    wsq = (f64 * f64).sum(0)
    rho = _TAP_CORR if taps > 1 else 0.0
    wvar = (1.0 - rho) * wsq + rho * wsum * wsum
    mu = np.zeros(coutp)
    var = np.zeros(coutp)
    if groups > 1:
        cg = cout // groups
        for g in range(groups):
            sl = slice(g * cg, (g + 1) * cg)
            mu[sl] = mu_in[g * cin_p:(g + 1) * cin_p] @ wsum[:, sl]
            var[sl] = var_in[g * cin_p:(g + 1) * cin_p] @ wvar[:, sl]
    else:
        mu = mu_in[:cin_p] @ wsum
        var = var_in[:cin_p] @ wvar
    b = np.zeros(coutp)
    if bias is not None:
        b[:cout] = np.asarray(bias, np.float64)
    return (mu + b)[:cout], np.maximum(var[:cout], 0.0)


def dw_moments(w9, bias, mu_in, var_in):
    w9 = np.asarray(w9, np.float64)
    wsum, wsq = w9.sum(0), (w9 * w9).sum(0)
    return (np.asarray(bias, np.float64) + mu_in * wsum,
            var_in * ((1.0 - _TAP_CORR) * wsq + _TAP_CORR * wsum * wsum))


def pointwise_moments(w, bias, mu_in, var_in):
    """w: (cout, cin) of a 1x1 conv over independent channels."""
    return np.asarray(bias, np.float64) + w @ mu_in, (w * w) @ var_in


def pool_moments(mu, var):
    """2x2 max-pool: the max of four ~ independent values."""
    return mu + 1.03 * np.sqrt(var), 0.49 * var


def rfstem_moments(mu_in, var_in, Ws, bs, blocks):
    """conv3x3 (Ws (8, 3, 3, 3), bs) + ReLU, then per block (Wd, bd, Wp, bp) a depthwise 3x3 + ReLU and a 1x1, ReLU between the
    blocks: (mean, var) in front of the last block's activation."""
    ws = np.asarray(Ws, np.float64)
    wsum, wsq = ws.sum((2, 3)), (ws * ws).sum((2, 3))                 # (8, 3)
    mu = np.asarray(bs, np.float64) + wsum @ mu_in
    var = ((1.0 - _TAP_CORR) * wsq + _TAP_CORR * wsum * wsum) @ var_in
    for Wd, bd, Wp, bp in blocks:
        c = np.asarray(Wd).shape[0]
        mu, var = act_moments(mu, var, ACT_RELU)
        mu, var = dw_moments(np.asarray(Wd, np.float64).reshape(c, 9).T, bd, mu, var)
        mu, var = act_moments(mu, var, ACT_RELU)
        mu, var = pointwise_moments(np.asarray(Wp, np.float64).reshape(-1, c), bp, mu, var)
    return mu, var
