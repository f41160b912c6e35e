"""CPU reference of the frame read-out (tsdf_present: what glfwSwapBuffers puts on the client's RGBA8 window, source/kinect_client.cpp:533,
or that picture as the wire's DXT1 blocks), as defined in include/rgbd_recon_hip.h.  numpy; the conversion in fp32, the encoder in integers,
every operation in the order the header states it.

* to_rgba8(fb_c, top_down): the float framebuffer [h][w][4] (row j = GL window row j) -> uint8 [h][w][4] in output row order.
* encode_dxt1(img8, diagonal=True): uint8 [h][w][>=3] in output row order -> uint8 [ceil(h/4) * ceil(w/4) * 8] blocks.
* present(fb_c, fmt, flags): the bytes one presented frame holds.
"""
import numpy as np

F = np.float32
RGBA8, DXT1 = 0, 1                  # TSDF_PRESENT_RGBA8 / TSDF_PRESENT_DXT1
TOP_DOWN = 1                        # TSDF_PRESENT_TOP_DOWN


def to_rgba8(fb_c, top_down=False):
    """u = (uint8) rint_half_even(min(max(v, 0), 1) * 255.0f), product in fp32, NaN -> 0, +-inf clamp; alpha like the colour channels"""
    v = np.asarray(fb_c, np.float32)
    assert v.ndim == 3 and v.shape[2] == 4
    with np.errstate(invalid="ignore"):
        v = np.clip(np.nan_to_num(v, nan=0.0, posinf=np.inf, neginf=-np.inf), F(0), F(1))
    p = v * F(255.0)
    assert p.dtype == np.float32
    out = np.rint(p).astype(np.uint8)
    return np.ascontiguousarray(out[::-1]) if top_down else out


def size_bytes(w, h, fmt):
    return w * h * 4 if fmt == RGBA8 else ((w + 3) // 4) * ((h + 3) // 4) * 8


def _blocks(img8):
    """[h][w][>=3] -> int32 [nby][nbx][16][3], texel i = 4 y + x, texels outside the image replicate the last column / row"""
    a = np.asarray(img8)
    h, w = a.shape[:2]
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    yy = np.minimum(np.arange(nby * 4), h - 1)
    xx = np.minimum(np.arange(nbx * 4), w - 1)
    p = a[yy][:, xx, :3].astype(np.int32)
    return p.reshape(nby, 4, nbx, 4, 3).transpose(0, 2, 1, 3, 4).reshape(nby, nbx, 16, 3)


def _expand565(c):
    """565 word -> [..., 3] 8-bit colour by bit replication (what the library's DXT1 decoder does)"""
    r5, g6, b5 = (c >> 11) & 31, (c >> 5) & 63, c & 31
    return np.stack([(r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)], -1)


def encode_dxt1(img8, diagonal=True):
    T = _blocks(img8)                                            # [nby][nbx][16][3]
    lo, hi = T.min(2), T.max(2)
    inset = (hi - lo) >> 4
    lo, hi = lo + inset, hi - inset
    A, B = hi.copy(), lo.copy()
    if diagonal:                                                 # r and b against g: a negative covariance swaps that channel's ends
        g = T[..., 1]
        for c in (0, 2):
            cov = 16 * (T[..., c] * g).sum(2) - T[..., c].sum(2) * g.sum(2)
            neg = cov < 0
            A[..., c] = np.where(neg, lo[..., c], hi[..., c])
            B[..., c] = np.where(neg, hi[..., c], lo[..., c])
    a565 = ((A[..., 0] >> 3) << 11) | ((A[..., 1] >> 2) << 5) | (A[..., 2] >> 3)
    b565 = ((B[..., 0] >> 3) << 11) | ((B[..., 1] >> 2) << 5) | (B[..., 2] >> 3)
    c0, c1 = np.maximum(a565, b565), np.minimum(a565, b565)
    p0, p1 = _expand565(c0), _expand565(c1)
    pal = np.stack([p0, p1, (2 * p0 + p1) // 3, (p0 + 2 * p1) // 3], 2)          # [nby][nbx][4][3]
    d = ((T[:, :, :, None, :] - pal[:, :, None, :, :]) ** 2).sum(-1)            # [nby][nbx][16][4]
    idx = d.argmin(-1).astype(np.uint64)                                       # (argmin: the lowest k among equals)
    word = (idx << (2 * np.arange(16, dtype=np.uint64))).sum(-1).astype(np.uint32)
    word = np.where(c0 == c1, np.uint32(0), word)
    out = np.zeros(T.shape[:2] + (8,), np.uint8)
    out[..., 0], out[..., 1] = c0 & 255, c0 >> 8
    out[..., 2], out[..., 3] = c1 & 255, c1 >> 8
    for k in range(4):
        out[..., 4 + k] = (word >> np.uint32(8 * k)) & np.uint32(255)
    return out.reshape(-1)


def present(fb_c, fmt=RGBA8, flags=0):
    img = to_rgba8(fb_c, bool(flags & TOP_DOWN))
    return img.reshape(-1) if fmt == RGBA8 else encode_dxt1(img)


def psnr(a, b):
    e = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    return 10.0 * np.log10(255.0 ** 2 / e.mean())
