"""The integer Conv (QModel.integer_conv) restated in NumPy int64 / float64 / float32: the
reference's q_matmul applied to the reference's im2col of the QUANTIZED input.

    cols_q[(b,oy,ox)][(ki,kj,ci)] = xq[b][ci][oy*sh-ph0+ki][ox*sw-pw0+kj]     padded cells = zx (0 if None)
    acc[r][n]  = sum_k cols_q[r][k] * Wq[n][ci][ki][kj]                       exact integers
    term       = zx*colsum_W[n] + zw*rowsum_cols[r] - K*zx*zw
    y[r][n]    = f32( f64(acc - term) * f64( f32(sx * sw) ) )
    out NCHW   = y + bias[n]                                                  one f32 add

Nothing here comes from the package under test."""
import numpy as np


def out_size(size, k, p0, p1, s):
    return (size - k + p0 + p1) // s + 1


def im2col_q(xq, kh, kw, pads, strides, zx):
    """cols int64 [n*ho*wo, kh*kw*c] (column order ki, kj, ci), ho, wo; pads = (ph0, pw0, ph1, pw1)."""
    xq = np.asarray(xq, dtype=np.int64)
    n, c, h, w = xq.shape
    ph0, pw0, ph1, pw1 = pads
    sh, sw = strides
    ho, wo = out_size(h, kh, ph0, ph1, sh), out_size(w, kw, pw0, pw1, sw)
    xp = np.pad(xq, ((0, 0), (0, 0), (ph0, ph1), (pw0, pw1)), constant_values=0 if zx is None else int(zx))
    cols = np.empty((n, ho, wo, kh, kw, c), dtype=np.int64)
    for ki in range(kh):
        for kj in range(kw):
            win = xp[:, :, ki:ki + sh * ho:sh, kj:kj + sw * wo:sw][:, :, :ho, :wo]  # [n, c, ho, wo]
            cols[:, :, :, ki, kj, :] = win.transpose(0, 2, 3, 1)
    return cols.reshape(n * ho * wo, kh * kw * c), ho, wo


def centred(xq, zx, wq, zw, pads, strides):
    """acc - term, int64 [rows, N], and (ho, wo)."""
    wq = np.asarray(wq, dtype=np.int64)
    kout, c, kh, kw = wq.shape
    cols, ho, wo = im2col_q(xq, kh, kw, pads, strides, zx)
    kk = kh * kw * c
    wm = wq.transpose(2, 3, 1, 0).reshape(kk, kout)
    acc = cols @ wm
    term = np.zeros((1, 1), dtype=np.int64)
    if zx is not None:
        term = term + np.int64(zx) * wm.sum(0)[None, :]
    if zw is not None:
        term = term + np.int64(zw) * cols.sum(1)[:, None]
    if zx is not None and zw is not None:
        term = term - np.int64(kk) * np.int64(zx) * np.int64(zw)
    return acc - term, ho, wo


def pre_bias(xq, zx, sx, wq, zw, sw, pads, strides):
    """y float32 [rows, N], ho, wo."""
    v, ho, wo = centred(xq, zx, wq, zw, pads, strides)
    scale = np.float32(np.float32(sx) * np.float32(sw))
    return (v.astype(np.float64) * np.float64(scale)).astype(np.float32), ho, wo


def qconv2d(xq, zx, sx, wq, zw, sw, bias, pads, strides):
    """out float32 NCHW."""
    y, ho, wo = pre_bias(xq, zx, sx, wq, zw, sw, pads, strides)
    n, kout = np.shape(xq)[0], np.shape(wq)[0]
    y = y.reshape(n, ho, wo, kout).transpose(0, 3, 1, 2)
    return (y + np.asarray(bias, dtype=np.float32).reshape(1, kout, 1, 1)).astype(np.float32)


def embed(xq, zx, sx, wq, sw, bias, cls, pos):
    """The patch embedding [n, hw + 1, N] of a patchify Conv (stride = kernel, no padding, weight
    without a zero point): out[b][0] = cls + pos[0], out[b][1 + t] = (y + bias) + pos[1 + t]."""
    kout, c, kh, kw = np.shape(wq)
    y, ho, wo = pre_bias(xq, zx, sx, wq, None, sw, (0, 0, 0, 0), (kh, kw))
    n, hw = np.shape(xq)[0], ho * wo
    bias, cls = np.asarray(bias, np.float32).reshape(kout), np.asarray(cls, np.float32).reshape(kout)
    pos = np.asarray(pos, np.float32).reshape(hw + 1, kout)
    out = np.empty((n, hw + 1, kout), dtype=np.float32)
    out[:, 0] = cls + pos[0]
    out[:, 1:] = (y.reshape(n, hw, kout) + bias) + pos[1:]
    return out


def brute(xq, zx, wq, zw, pads, strides):
    """Six-loop integer convolution of (x - zx) and (w - zw), int64 [rows, N]: padded cells
    contribute (zx - zx) = 0."""
    xq = np.asarray(xq, dtype=np.int64)
    wq = np.asarray(wq, dtype=np.int64)
    n, c, h, w = xq.shape
    kout, _, kh, kw = wq.shape
    ph0, pw0, ph1, pw1 = pads
    sh, sw = strides
    ho, wo = out_size(h, kh, ph0, ph1, sh), out_size(w, kw, pw0, pw1, sw)
    zx = 0 if zx is None else int(zx)
    zw = 0 if zw is None else int(zw)
    out = np.zeros((n, ho, wo, kout), dtype=np.int64)
    for b in range(n):
        for oy in range(ho):
            for ox in range(wo):
                for ci in range(c):
                    for ki in range(kh):
                        for kj in range(kw):
                            iy, ix = oy * sh - ph0 + ki, ox * sw - pw0 + kj
                            if 0 <= iy < h and 0 <= ix < w:
                                out[b, oy, ox, :] += (xq[b, ci, iy, ix] - zx) * (wq[:, ci, ki, kj] - zw)
    return out.reshape(n * ho * wo, kout)
