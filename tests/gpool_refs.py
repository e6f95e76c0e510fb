"""fp64 / numpy references of the global pooling branch, written from the formulas and not from
``ConvStack.forward_torch``.  Activations are NCHW arrays (B, C, S, S).

    P[b, 0, c] = (sum_p Y[b, c, p]) * inv          inv = float32(1 / (S * S))
    P[b, 1, c] = max_p Y[b, c, p]                   a[b, c] = lowest p attaining it
    g[b, :]    = P[b].reshape(2C) @ Wg              Wg (2C, C)
    Y2         = relu(conv(Y1, W2) + b2 + Yin + g[b, :, None, None])
"""
import numpy as np


def inv_np(S):
    return np.float64(np.float32(1.0 / (S * S)))


def pool(y):
    """(P (B, 2, C), a (B, C)): mean (sum times the fp32-rounded 1 / NP) and max; np.argmax returns the
    first, i.e. lowest, index among equal maxima."""
    y = np.asarray(y, dtype=np.float64)
    B, C, S, _ = y.shape
    flat = y.reshape(B, C, S * S)
    a = flat.argmax(2)
    P = np.stack([flat.sum(2) * inv_np(S), np.take_along_axis(flat, a[:, :, None], 2)[:, :, 0]], 1)
    return P, a


def gate(P, Wg):
    return P.reshape(P.shape[0], -1) @ np.asarray(Wg, dtype=np.float64)


def conv(x, w, b=None):
    """'same' cross-correlation, stride 1: x (B, Ci, S, S), w (Co, Ci, K, K) OIHW."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = w.shape[2]
    S = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (K // 2, K // 2), (K // 2, K // 2)))
    out = np.zeros((x.shape[0], w.shape[0], S, S))
    for u in range(K):
        for v in range(K):
            out += np.einsum("birc,oi->borc", xp[:, :, u:u + S, v:v + S], w[:, :, u, v])
    return out if b is None else out + np.asarray(b, dtype=np.float64)[None, :, None, None]


def conv_dgrad(dz, w):
    """Gradient of ``conv`` with respect to its input."""
    w = np.asarray(w, dtype=np.float64)
    return conv(dz, w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def conv_wgrad(x, dz, K):
    """Gradient of ``conv`` with respect to its weights (Co, Ci, K, K)."""
    S = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (K // 2, K // 2), (K // 2, K // 2)))
    out = np.zeros((dz.shape[1], x.shape[1], K, K))
    for u in range(K):
        for v in range(K):
            out[:, :, u, v] = np.einsum("borc,birc->oi", dz, xp[:, :, u:u + S, v:v + S])
    return out


def block_forward(yin, w1, b1, w2, b2, Wg=None):
    """A residual block on its input ``yin``: (Y1, Y2, P, a); ``Wg=None`` is a block without the branch."""
    y1 = np.maximum(conv(yin, w1, b1), 0.0)
    skip = np.asarray(yin, dtype=np.float64)
    P = a = None
    if Wg is not None:
        P, a = pool(y1)
        skip = skip + gate(P, Wg)[:, :, None, None]
    return y1, np.maximum(conv(y1, w2, b2) + skip, 0.0), P, a


def trunk_forward(x, weights, biases, gates):
    """A residual ConvStack: ``gates[j]`` is block j's Wg or None."""
    y = np.maximum(conv(x, weights[0], biases[0]), 0.0)
    for j in range((len(weights) - 1) // 2):
        l = 2 * j + 1
        y = block_forward(y, weights[l], biases[l], weights[l + 1], biases[l + 1], gates[j])[1]
    return y


def pool_backward(dP, a, S):
    """Gradient of ``pool`` with respect to its input: dP[b, 0, c] * inv at every pixel plus dP[b, 1, c] at
    pixel a[b, c] alone."""
    B, _, C = dP.shape
    out = np.repeat((dP[:, 0] * inv_np(S))[:, :, None], S * S, 2)
    hit = np.arange(S * S)[None, None, :] == a[:, :, None]
    return (out + np.where(hit, dP[:, 1][:, :, None], 0.0)).reshape(B, C, S, S)


def block_backward(yin, w1, b1, w2, b2, Wg, dy2):
    """Analytic backward of ``block_forward`` from the gradient ``dy2`` at the block's output (after its
    ReLU): dict of the gradients with respect to w1, b1, w2, b2, Wg and the block input."""
    y1, y2, P, a = block_forward(yin, w1, b1, w2, b2, Wg)
    S = y1.shape[2]
    dz2 = dy2 * (y2 > 0)
    dg = dz2.sum((2, 3))
    dWg = P.reshape(P.shape[0], -1).T @ dg
    dP = (dg @ np.asarray(Wg, dtype=np.float64).T).reshape(P.shape)
    dz1 = (conv_dgrad(dz2, w2) + pool_backward(dP, a, S)) * (y1 > 0)
    return dict(w1=conv_wgrad(np.asarray(yin, dtype=np.float64), dz1, w1.shape[2]), b1=dz1.sum((0, 2, 3)),
                w2=conv_wgrad(y1, dz2, w2.shape[2]), b2=dz2.sum((0, 2, 3)), Wg=dWg,
                yin=conv_dgrad(dz1, w1) + dz2)
