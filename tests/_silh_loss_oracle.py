"""The silhouette loss head in float64, restated from its definition (csrc/silh_loss_device.h): per pixel, with s the
silhouette score of channel 1 and z0 the value of channel 0 (the fp32 number 1 - s the forward stored, or 1 - s),

    p = softmax(z0, s),  L = w_t (1 - p_t)^gamma (-log p_t),  k = dL/ds = +-2 q p0 p1 (+ for t = 1),
    q = w_t (gamma (1 - p_t)^(gamma - 1) log p_t - (1 - p_t)^gamma / p_t);

a label outside {0, 1} gives L = k = 0; NaN scores give NaN."""
import numpy as np

FOCAL_W2 = (0.3, 2.0)       # the first two entries of the class-weight table (focal_loss.py:22-40)


def silh_loss(s, labels, gamma=0.0, weights=None, z0=None):
    """s, labels (and z0, default 1 - s) of one shape -> (L, k) float64 of that shape."""
    s = np.asarray(s, np.float64)
    z0 = 1.0 - s if z0 is None else np.asarray(z0, np.float64)
    t = np.asarray(labels, np.int64)
    valid = (t == 0) | (t == 1)
    tt = np.where(valid, t, 0)
    mx = np.maximum(z0, s)
    e0, e1 = np.exp(z0 - mx), np.exp(s - mx)
    p0, p1 = e0 / (e0 + e1), e1 / (e0 + e1)
    pt = np.where(tt == 1, p1, p0)
    w = np.ones_like(pt) if weights is None else np.where(tt == 1, float(weights[1]), float(weights[0]))
    om, lg = 1.0 - pt, np.log(pt)
    with np.errstate(invalid="ignore", divide="ignore"):
        L = w * om ** gamma * (-lg)
        dpow = gamma * om ** (gamma - 1.0) if gamma != 0 else np.zeros_like(om)
        q = w * (dpow * lg - om ** gamma / pt)
    k = np.where(tt == 1, 1.0, -1.0) * 2.0 * q * p0 * p1
    return np.where(valid, L, 0.0), np.where(valid, k, 0.0)


def confusion(silh, labels):
    """(3, 2) int64 counts of (label, arg-max of the two channels), row 2 = labels outside {0, 1}; channel 0 on a tie and
    on NaN (np.argmax's order on a NaN pair)."""
    silh = np.asarray(silh)
    pred = (silh[..., 1] > silh[..., 0]).astype(np.int64).reshape(-1)
    t = np.asarray(labels, np.int64).reshape(-1)
    row = np.where((t == 0) | (t == 1), t, 2)
    return np.bincount(row * 2 + pred, minlength=6).reshape(3, 2)
