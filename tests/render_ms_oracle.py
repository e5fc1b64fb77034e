"""The multisampled renderer's contract (ofx_render_raster_ms / ofx_render_shade_ms, include/ofx.h) on
top of tests/render_oracle.py.  Nothing here imports the product, and the rasteriser is not copied:

  * edge functions, the ownership rule and the depth formula are translation-invariant, so sample plane s of the key
    buffer is `render_oracle.raster` on the coordinates shifted by (128 - ox_s, 128 - oy_s): the sample then sits
    where that rasteriser has its pixel centre.  Its pixel box is computed, and clamped to the screen, after the shift;
  * the resolve: every face among a pixel's samples is shaded at the ray through the pixel's CENTRE (render_oracle.shade
    without its final quantisation), a sample's colour is that colour clamped to [0, 1] or the background, the pixel
    is floor(255 (sum_s c_s) / S + 0.5) with the sum in sample order in float64.
"""
import math

import numpy as np

import render_oracle as O

# sub-pixel units (1/256 pixel) from the pixel's origin (256 i, 256 j)
_O16 = [(1, 1), (-1, -3), (-3, 2), (4, -1), (-5, -2), (2, 5), (5, 3), (3, -5),
        (-2, 6), (0, -7), (-4, -6), (-6, 4), (-8, 0), (7, -4), (6, 7), (-7, -8)]
OFFSETS = {
    1: [(128, 128)],
    4: [(96, 32), (224, 96), (32, 160), (160, 224)],
    16: [(128 + 16 * a, 128 + 16 * b) for a, b in _O16],
}


def raster_ms(sxy, depth, faces, size, offsets):
    """(keys [size, size, S] uint64, dropped count) of one mesh in one view."""
    sxy = np.asarray(sxy, np.int64)
    live = sxy[:, 0] != O.DROPPED
    keys = np.empty((size, size, len(offsets)), np.uint64)
    dropped = 0
    for s, (ox, oy) in enumerate(offsets):
        shifted = sxy.copy()
        shifted[live, 0] += O.HALF - int(ox)
        shifted[live, 1] += O.HALF - int(oy)
        keys[:, :, s], dropped = O.raster(shifted, depth, faces, size)
    return keys, dropped


def face_colours(verts, faces, ids, pose, size, centre, scale, background=1.0, **material):
    """float64 [3][...]: the unquantised, unclamped colour of face ids[y, x, ...] at the centre ray of pixel (x, y);
    ids [size, size] or [size, size, S], -1 background (left at 0 here).  The body of render_oracle.shade."""
    S = O.shade_params(background, **material)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.asarray(ids, np.int64)
    pose = np.asarray(pose, np.float64)
    tan_half = math.tan(O.YFOV / 2.0)
    hit = ids >= 0
    tri = faces[np.where(hit, ids, 0)]
    shape = ids.shape
    with np.errstate(all='ignore'):
        P = [[(v[tri[..., k], a] - centre[a]) / scale for a in range(3)] for k in range(3)]
        eye = [pose[0, 3], pose[1, 3], pose[2, 3]]
        zax = [pose[0, 2], pose[1, 2], pose[2, 2]]
        ys, xs = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing='ij')
        u = ((xs + 0.5) / float(size) * 2.0 - 1.0) * tan_half
        w = (1.0 - (ys + 0.5) / float(size) * 2.0) * tan_half
        if ids.ndim == 3:
            u, w = u[:, :, None], w[:, :, None]
        dirv = [np.broadcast_to((pose[a, 0] * u + pose[a, 1] * w) - pose[a, 2], shape) for a in range(3)]
        n = O._cross([P[1][a] - P[0][a] for a in range(3)], [P[2][a] - P[0][a] for a in range(3)])
        den = O._dot(n, dirv)
        t = O._dot(n, [P[0][a] - eye[a] for a in range(3)]) / np.where(den != 0.0, den, 1.0)
        pos = [np.where(den != 0.0, eye[a] + t * dirv[a], ((P[0][a] + P[1][a]) + P[2][a]) / 3.0) for a in range(3)]
        lv = [eye[a] - pos[a] for a in range(3)]
        d2 = O._dot(lv, lv)
        d2 = np.where(d2 >= 1e-12, d2, 1e-12)
        inv = 1.0 / np.sqrt(d2)
        V = [lv[a] * inv for a in range(3)]
        nn = O._dot(n, n)
        ninv = 1.0 / np.sqrt(np.where(nn > 0.0, nn, 1.0))
        N = [np.where(nn > 0.0, n[a] * ninv, V[a]) for a in range(3)]
        flip = O._dot(N, V) < 0.0
        N = [np.where(flip, -N[a], N[a]) for a in range(3)]
        col = [np.zeros(shape) for _ in range(3)]
        Lz = [np.full(shape, zax[a]) for a in range(3)]
        O._light(S, N, V, Lz, np.full(shape, S['i_dir']), col)
        O._light(S, N, V, V, S['i_point'] / d2, col)
        sa = O._dot(zax, V) * S['spot_scale'] + S['spot_offset']
        sa = np.where(sa > 0.0, np.where(sa < 1.0, sa, 1.0), 0.0)
        O._light(S, N, V, V, (S['i_spot'] / d2) * (sa * sa), col)
    return col


def resolve(colours, hit, bg):
    """uint8 [size, size, 3] from per-sample colours [3][size, size, S], the hit mask and the background rgb."""
    S = hit.shape[2]
    out = np.empty(hit.shape[:2] + (3,), np.uint8)
    with np.errstate(all='ignore'):
        for c in range(3):
            q = np.where(hit, colours[c], bg[c])
            q = np.where(q > 0.0, np.where(q < 1.0, q, 1.0), 0.0)        # per sample; a NaN becomes 0
            acc = q[:, :, 0]
            for s in range(1, S):
                acc = acc + q[:, :, s]
            out[..., c] = np.floor(255.0 * (acc / float(S)) + 0.5).astype(np.uint8)
    return out


def shade_ms(verts, faces, ids, pose, size, centre, scale, background=1.0, **material):
    """uint8 [size, size, 3] of one mesh in one view from its per-sample id buffer (ids [size, size, S])."""
    ids = np.asarray(ids, np.int64)
    col = face_colours(verts, faces, ids, pose, size, centre, scale, background, **material)
    return resolve(col, ids >= 0, O.shade_params(background, **material)['bg'])
