"""CPU reference of the GUI's "Show textures" windows (tsdf_draw_sensor_texture; source/kinect_client.cpp:483-515 drawn by the ImGui back-end's
array mode, external/imgui-1.49/imgui_impl_glfw_glb.cpp:68-74,111-124,260-285), as defined in include/rgbd_recon_hip.h.  numpy, fp32
throughout, every operation in the order the header states it.

* texel_vec4(type, layer): the seven texel-to-vec4 rules, on one layer as the library returns it.
* draw(type, layer, rect, clip, fb_c): coverage, Frag_UV, the quarter turn, the filter of the type, the blend and the scissor box, on a copy
  of the framebuffer colour [h][w][4] (row j = GL window row j).  Depth is never touched.
"""
import numpy as np

import overlay_reference as O

F = np.float32
ROT_C = np.array([0xb33bbd2e], np.uint32).view(np.float32)[0]     # cosf(1.5707964f) = -4.37113883e-08
ROT_S = F(1.0)                                                     # sinf(1.5707964f)
NAMES = ["Color", "Depth", "Quality", "Normals", "Silhouette", "Orig Depth", "LAB colors"]
NEAREST = {1, 5}                                                   # NetKinectArray.cpp:147-188: depth_b and depth2; everything else LINEAR


def texel_vec4(type, layer):
    """type 0: uint8 [ch][cw][3] (RGB8 -> (rgb / 255, 1)) or [ch][cw][4] (the decoded RGBA8 -> rgba / 255); 1: [h][w][2] -> (r, g, 0, 1), or
    [h][w] -- the frame slot's depth.r alone -- -> (r, 0, 0, 1); 2, 5: [h][w] -> (L, L, L, 1); 3, 6: [h][w][3] -> (rgb, 1); 4: [h][w] -> (r, 0, 0, 1)"""
    a = np.asarray(layer)
    h, w = a.shape[:2]
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = F(1)
    if type == 0:
        assert a.dtype == np.uint8
        out[..., :a.shape[2]] = a.astype(np.float32) / F(255)
    elif type == 1:
        a = a.astype(np.float32)
        if a.ndim == 3:
            out[..., :2] = a[..., :2]
        else:
            out[..., 0] = a
    elif type in (2, 5):
        out[..., :3] = a.astype(np.float32)[..., None]
    elif type in (3, 6):
        out[..., :3] = a.astype(np.float32)[..., :3]
    elif type == 4:
        out[..., 0] = a.astype(np.float32)
    else:
        raise ValueError(type)
    return out


def scissor_box(clip, view):
    """(sx, sy, sw, sh) of glScissor at imgui_impl_glfw_glb.cpp:123; None: the whole view"""
    w, h = view
    if clip is None:
        return 0, 0, w, h
    x, y, z, ww = [F(v) for v in clip]
    t = lambda v: int(np.clip(v, F(-2.0**30), F(2.0**30)))
    return t(x), t(F(h) - ww), t(z - x), t(ww - y)


def coverage(rect, clip, view):
    """-> (mask [h][w], cx [w], cy [h])"""
    w, h = view
    pminx, pminy, pmaxx, pmaxy = [F(v) for v in rect]
    cx = np.arange(w, dtype=np.float32) + F(0.5)
    cy = F(h) - (np.arange(h, dtype=np.float32) + F(0.5))
    inx = (pminx <= cx) & (cx < pmaxx)
    iny = (pminy <= cy) & (cy < pmaxy)
    sx, sy, sw, sh = scissor_box(clip, view)
    i, j = np.arange(w), np.arange(h)
    inx &= (i >= sx) & (i < sx + max(sw, 0))
    iny &= (j >= sy) & (j < sy + max(sh, 0))
    return iny[:, None] & inx[None, :], cx, cy


def frag_uv(rect, cx, cy):
    pminx, pminy, pmaxx, pmaxy = [F(v) for v in rect]
    u = (cx - pminx) / (pmaxx - pminx)
    v = (cy - pminy) / (pmaxy - pminy)
    return np.broadcast_to(u[None, :], (cy.size, cx.size)).astype(np.float32), np.broadcast_to(v[:, None], (cy.size, cx.size)).astype(np.float32)


def rotate(u, v, c=ROT_C, s=ROT_S):
    """uv -= .5; uv = mat2(c, -s, s, c) * uv; uv += .5 -- products first, then the sum"""
    c, s = F(c), F(s)
    u, v = (u - F(0.5)).astype(np.float32), (v - F(0.5)).astype(np.float32)
    ru = ((c * u).astype(np.float32) + (s * v).astype(np.float32)).astype(np.float32)
    rv = (((-s) * u).astype(np.float32) + (c * v).astype(np.float32)).astype(np.float32)
    return (ru + F(0.5)).astype(np.float32), (rv + F(0.5)).astype(np.float32)


def axis_nearest(u, n):
    return np.clip(np.floor(np.asarray(u, np.float32) * F(n)), 0, n - 1).astype(np.int64)


def sample(src, u, v, nearest):
    """texture(array, (u, v, layer)) of the layer's vec4 image src [sh][sw][4]"""
    src = np.asarray(src, np.float32)
    sh, sw = src.shape[:2]
    if nearest:
        return src[axis_nearest(v, sh), axis_nearest(u, sw)]
    x0, x1, ax = O.axis_linear(u, sw)
    y0, y1, ay = O.axis_linear(v, sh)
    ax, ay = ax[..., None], ay[..., None]
    return O.lerp(O.lerp(src[y0, x0], src[y0, x1], ax), O.lerp(src[y1, x0], src[y1, x1], ax), ay)


def blend(s, d):
    """SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels; a sample with alpha == 1 replaces the pixel"""
    a = s[..., 3:4]
    k = (F(1) - a).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = ((s * a).astype(np.float32) + (d * k).astype(np.float32)).astype(np.float32)
    return np.where(a == F(1), s, mixed).astype(np.float32)


def draw(type, layer, rect, clip, fb_c, c=ROT_C, s=ROT_S):
    fb = np.array(fb_c, np.float32, copy=True)
    h, w = fb.shape[:2]
    mask, cx, cy = coverage(rect, clip, (w, h))
    u, v = frag_uv(rect, cx, cy)
    ru, rv = rotate(u, v, c, s)
    smp = sample(texel_vec4(type, layer), ru, rv, type in NEAREST)
    fb[mask] = blend(smp, fb)[mask]
    return fb


def view_size(width, depth_res):
    """ImVec2(width, width / aspect), aspect = float(res.y) / res.x (kinect_client.cpp:502-509)"""
    aspect = F(depth_res[1]) / F(depth_res[0])
    return F(width), F(width) / aspect
