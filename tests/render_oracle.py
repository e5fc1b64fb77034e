"""numpy / Python-integer restatement of the renderer's contract (include/ofx.h "rendering", csrc/ofx_render.hip,
octfusion_amd.render).  Nothing here imports the product.

  * views: the 20 eye positions from the dodecahedron's closed form, look_at poses, the rigid inverse;
  * normalise + project in float64: screen position snapped to 1/256 pixel (int), window depth (float64), dropped
    vertices;
  * the integer rasteriser: int64 edge functions at pixel centres, top-left rule, both windings, float64 depth in the
    kernel's operation order, 64-bit keys resolved by minimum;
  * flat two-sided glTF metallic-roughness shading under three lights at the camera, float64, the kernel's order.

Every float64 operation is a separately rounded numpy operation in the order the kernel performs it, so on the same
snapped coordinates the key buffer is equal bit for bit and the shading differs only where libm's sqrt / division do.
"""
import math

import numpy as np

SUB, HALF = 256, 128
GUARD = float(2 ** 26)
DROPPED = -2 ** 31
EMPTY = 2 ** 64 - 1
YFOV = math.pi / 3.0
ZNEAR, ZFAR = 0.05, 100.0
MATERIAL = dict(base_color=(0.3, 0.3, 0.3), metallic=0.2, roughness=0.8, directional=3.0, point=6.0, spot=3.0,
                spot_inner=math.pi / 16, spot_outer=math.pi / 6)


# ---- cameras -------------------------------------------------------------------------------------------------------
def fid_views():
    s5 = 5.0 ** 0.5
    a = ((5.0 + s5) / 10.0) ** 0.5
    r = 2.0 * math.tan(math.pi / 10.0)
    R = 2.0 * ((5.0 - s5) / 10.0) ** 0.5
    b = a - r
    deg = math.pi / 180.0
    top = [(r * math.cos((36 + 72 * k) * deg), r * math.sin((36 + 72 * k) * deg), a) for k in range(5)]
    mid = [(R * math.cos((-36 + 36 * k) * deg), R * math.sin((-36 + 36 * k) * deg), b * (-1) ** k) for k in range(10)]
    bot = [(r * math.cos(72 * k * deg), r * math.sin(72 * k * deg), -a) for k in range(5)]
    return 2.0 * np.array(top + mid + bot, np.float64)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, np.asarray(up, np.float64))
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = s, u, -f, eye
    return pose


def view_matrix(pose):
    """[3, 4]: the rigid inverse R^T, -R^T t."""
    pose = np.asarray(pose, np.float64)
    R, t = pose[:3, :3], pose[:3, 3]
    m = np.empty((3, 4))
    m[:, :3] = R.T
    for i in range(3):
        m[i, 3] = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
    return m


# ---- normalise + project -------------------------------------------------------------------------------------------
def normalization(verts, normalize=True):
    """(centre [3], scale) of one mesh: bounding-box centre and the largest distance from it, finite vertices only."""
    if not normalize:
        return np.zeros(3), 1.0
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    v32 = v32[np.isfinite(v32).all(1)]
    if len(v32) == 0:
        return np.zeros(3), 1.0
    lo, hi = v32.min(0).astype(np.float64), v32.max(0).astype(np.float64)
    c = (lo + hi) * 0.5
    d = v32.astype(np.float64) - c
    m = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    return c, (math.sqrt(m) if m > 0 else 1.0)


def project(verts, pose, size, centre, scale, znear=ZNEAR, zfar=ZFAR):
    """(sxy [N, 2] int64 with DROPPED in x for a dropped vertex, depth [N] float64, real-valued fx, fy)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    M = view_matrix(pose)
    focal = 1.0 / math.tan(YFOV / 2.0)
    half_units = float(size) * HALF
    dep_a = ((zfar + znear) / (zfar - znear) + 1.0) * 0.5
    dep_b = (zfar * znear) / (zfar - znear)
    with np.errstate(all='ignore'):
        p = (v - centre) / scale
        e = [((M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2]) + M[i, 3] for i in range(3)]
        w = -e[2]
        fx = ((e[0] * focal) / w + 1.0) * half_units
        fy = (1.0 - (e[1] * focal) / w) * half_units
        d = dep_a - dep_b / w
        ok = (w >= znear) & (np.abs(fx) <= GUARD) & (np.abs(fy) <= GUARD) & (np.abs(d) <= np.finfo(np.float64).max)
        sx = np.where(ok, np.rint(np.where(ok, fx, 0.0)), DROPPED).astype(np.int64)
        sy = np.where(ok, np.rint(np.where(ok, fy, 0.0)), 0).astype(np.int64)
    return np.stack([sx, sy], 1), np.where(ok, d, 0.0), fx, fy


# ---- the integer rasteriser ----------------------------------------------------------------------------------------
def _owns(ax, ay, bx, by):
    return by < ay or (by == ay and bx > ax)


def _floor_div(a, b):
    return a // b            # Python's // floors


def raster(sxy, depth, faces, size):
    """(keys [size, size] uint64, dropped count) of one mesh in one view.  sxy [N, 2] integers (x == DROPPED: dropped),
    depth [N] float64, faces [F, 3]."""
    sxy = np.asarray(sxy, np.int64)
    depth = np.asarray(depth, np.float64)
    keys = np.full((size, size), EMPTY, np.uint64)
    dropped = 0
    for f, (ia, ib, ic) in enumerate(np.asarray(faces, np.int64).tolist()):
        ax, ay = int(sxy[ia, 0]), int(sxy[ia, 1])
        bx, by = int(sxy[ib, 0]), int(sxy[ib, 1])
        cx, cy = int(sxy[ic, 0]), int(sxy[ic, 1])
        if DROPPED in (ax, bx, cx):
            dropped += 1
            continue
        za, zb, zc = depth[ia], depth[ib], depth[ic]
        area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area2 == 0:
            continue
        if area2 < 0:
            bx, by, cx, cy, zb, zc, area2 = cx, cy, bx, by, zc, zb, -area2
        x0 = max(_floor_div(min(ax, bx, cx) - HALF + SUB - 1, SUB), 0)
        y0 = max(_floor_div(min(ay, by, cy) - HALF + SUB - 1, SUB), 0)
        x1 = min(_floor_div(max(ax, bx, cx) - HALF, SUB), size - 1)
        y1 = min(_floor_div(max(ay, by, cy) - HALF, SUB), size - 1)
        if x0 > x1 or y0 > y1:
            continue
        px = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB + HALF)[None, :]
        py = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB + HALF)[:, None]
        ea = (cx - bx) * (py - by) - (cy - by) * (px - bx)
        eb = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
        ec = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        inside = (((ea > 0) | ((ea == 0) & _owns(bx, by, cx, cy))) &
                  ((eb > 0) | ((eb == 0) & _owns(cx, cy, ax, ay))) &
                  ((ec > 0) | ((ec == 0) & _owns(ax, ay, bx, by))))
        if not inside.any():
            continue
        s = (ea.astype(np.float64) * za + eb.astype(np.float64) * zb) + ec.astype(np.float64) * zc
        q = (s / float(area2)) * 4294967296.0
        q = np.where(q >= 0.0, q, 0.0)
        q = np.where(q > 4294967295.0, 4294967295.0, q)
        key = (q.astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        box = keys[y0:y1 + 1, x0:x1 + 1]
        box[inside] = np.minimum(box[inside], key[inside])
    return keys, dropped


def coverage(tri, size):
    """Boolean [size, size] coverage of one triangle ((ax, ay), (bx, by), (cx, cy)) in sub-pixel integers."""
    sxy = np.asarray(tri, np.int64).reshape(3, 2)
    keys, _ = raster(sxy, np.zeros(3), [[0, 1, 2]], size)
    return keys != np.uint64(EMPTY)


def split_keys(keys):
    """(ids int32 with -1 for background, quantised depth as integers)."""
    keys = np.asarray(keys, np.uint64)
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids[keys == np.uint64(EMPTY)] = -1
    return ids.astype(np.int32), (keys >> np.uint64(32)).astype(np.int64)


# ---- shading -------------------------------------------------------------------------------------------------------
def shade_params(background=1.0, **material):
    m = dict(MATERIAL, **material)
    ci, co = math.cos(m['spot_inner']), math.cos(m['spot_outer'])
    scale = 1.0 / max(0.001, ci - co)
    return dict(base=np.broadcast_to(np.asarray(m['base_color'], np.float64), (3,)), metallic=float(m['metallic']),
                roughness=float(m['roughness']), i_dir=float(m['directional']), i_point=float(m['point']),
                i_spot=float(m['spot']), spot_scale=scale, spot_offset=-co * scale,
                bg=np.broadcast_to(np.asarray(background, np.float64), (3,)))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _light(S, N, V, L, radiance, out):
    """out[c] += radiance * N.L * (diffuse + specular), where N.L > 0 and radiance > 0 (arrays over pixels)."""
    nl = _dot(N, L)
    hs = [L[k] + V[k] for k in range(3)]
    hh = _dot(hs, hs)
    on = (nl > 0.0) & (radiance > 0.0) & (hh > 0.0)
    inv = 1.0 / np.sqrt(np.where(hh > 0.0, hh, 1.0))
    H = [hs[k] * inv for k in range(3)]
    nv, nh = np.abs(_dot(N, V)), _dot(N, H)
    x = 1.0 - _dot(V, H)
    x = np.where(x > 0.0, x, 0.0)
    x2 = x * x
    x5 = (x2 * x2) * x
    al = S['roughness'] * S['roughness']
    a2 = al * al
    dd = (nh * nh) * (a2 - 1.0) + 1.0
    D = np.where(nh > 0.0, a2 / ((math.pi * dd) * dd), 0.0)
    vis = 1.0 / ((nl + np.sqrt(a2 + (1.0 - a2) * (nl * nl))) * (nv + np.sqrt(a2 + (1.0 - a2) * (nv * nv))))
    dv, rn = D * vis, radiance * nl
    for c in range(3):
        f0 = 0.04 * (1.0 - S['metallic']) + S['base'][c] * S['metallic']
        cd = S['base'][c] * (1.0 - S['metallic'])
        F = f0 + (1.0 - f0) * x5
        out[c] = np.where(on, out[c] + rn * ((1.0 - F) * (cd / math.pi) + F * dv), out[c])


def shade(verts, faces, ids, pose, size, centre, scale, background=1.0, **material):
    """uint8 [size, size, 3] of one mesh in one view from its id buffer (ids [size, size], -1 background)."""
    S = shade_params(background, **material)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.asarray(ids, np.int64)
    pose = np.asarray(pose, np.float64)
    tan_half = math.tan(YFOV / 2.0)
    hit = ids >= 0
    tri = faces[np.where(hit, ids, 0)]                                     # [size, size, 3]
    with np.errstate(all='ignore'):
        P = [[(v[tri[..., k], a] - centre[a]) / scale for a in range(3)] for k in range(3)]
        eye = [pose[0, 3], pose[1, 3], pose[2, 3]]
        zax = [pose[0, 2], pose[1, 2], pose[2, 2]]
        ys, xs = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing='ij')
        u = ((xs + 0.5) / float(size) * 2.0 - 1.0) * tan_half
        w = (1.0 - (ys + 0.5) / float(size) * 2.0) * tan_half
        dirv = [(pose[a, 0] * u + pose[a, 1] * w) - pose[a, 2] for a in range(3)]
        n = _cross([P[1][a] - P[0][a] for a in range(3)], [P[2][a] - P[0][a] for a in range(3)])
        den = _dot(n, dirv)
        t = _dot(n, [P[0][a] - eye[a] for a in range(3)]) / np.where(den != 0.0, den, 1.0)
        pos = [np.where(den != 0.0, eye[a] + t * dirv[a], ((P[0][a] + P[1][a]) + P[2][a]) / 3.0) for a in range(3)]
        lv = [eye[a] - pos[a] for a in range(3)]
        d2 = _dot(lv, lv)
        d2 = np.where(d2 >= 1e-12, d2, 1e-12)
        inv = 1.0 / np.sqrt(d2)
        V = [lv[a] * inv for a in range(3)]
        nn = _dot(n, n)
        ninv = 1.0 / np.sqrt(np.where(nn > 0.0, nn, 1.0))
        N = [np.where(nn > 0.0, n[a] * ninv, V[a]) for a in range(3)]
        flip = _dot(N, V) < 0.0
        N = [np.where(flip, -N[a], N[a]) for a in range(3)]
        col = [np.zeros((size, size)) for _ in range(3)]
        Lz = [np.full((size, size), zax[a]) for a in range(3)]
        _light(S, N, V, Lz, np.full((size, size), S['i_dir']), col)
        _light(S, N, V, V, S['i_point'] / d2, col)
        sa = _dot(zax, V) * S['spot_scale'] + S['spot_offset']
        sa = np.where(sa > 0.0, np.where(sa < 1.0, sa, 1.0), 0.0)
        _light(S, N, V, V, (S['i_spot'] / d2) * (sa * sa), col)
        out = np.empty((size, size, 3), np.uint8)
        for c in range(3):
            q = np.where(hit, col[c], S['bg'][c])
            q = np.where(q > 0.0, np.where(q < 1.0, q, 1.0), 0.0)
            out[..., c] = np.floor(255.0 * q + 0.5).astype(np.uint8)
    return out
