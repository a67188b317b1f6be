"""BatchNorm folding (float64 math; the packers store float32)."""
import numpy as np


def _bn_affine(sd, key, eps):
    g = np.asarray(sd[key + '.weight'], np.float64)
    b = np.asarray(sd[key + '.bias'], np.float64)
    m = np.asarray(sd[key + '.running_mean'], np.float64)
    v = np.asarray(sd[key + '.running_var'], np.float64)
    s = g / np.sqrt(v + eps)
    return s, b - m * s


def _fold(W, bias, scale, shift):
    """BN(conv(x)+bias) -> conv'(x)+bias'."""
    W = np.asarray(W, np.float64) * scale[:, None, None, None]
    b0 = np.zeros(W.shape[0]) if bias is None else np.asarray(bias, np.float64)
    return W, b0 * scale + shift
