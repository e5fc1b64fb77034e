"""Shaded views of meshes on the device, and the image folders of the reference's FID protocol.

Replaces the reference's host renderer (metrics/generate_synth_image.py, generate_dataset_for_fid.py ->
utils/render_utils.py:14-23 generate_image_for_fid -> utils/render/render.py:10-41 render_mesh): every mesh is scaled to
the unit sphere (utils/util.py:91-100), seen from 20 fixed views at 299 x 299 under three lights at the camera, and
saved as ``view_<j>/<name>.png``.  The reference draws with pyrender over EGL; here three HIP stages
(csrc/ofx_render.hip: project, raster, shade) draw straight from the device meshes ``mesh.marching_cubes`` returns.

The renderer is the project's own and deterministic -- coverage and visibility are exact integer functions of the
screen coordinates snapped to 1/256 pixel -- and its parity with pyrender is unpinned: FID compares
two image sets, so draw BOTH the generated set and the dataset set with it.  The FID number itself is computed outside
the project (the folders feed the reference's metrics/calc_fid.py unchanged).

``samples`` = 4 or 16 draws multisampled: coverage and depth per sample, one flat shade per face and pixel at the
pixel-centre ray, the samples averaged and quantised once.  The reference's pyrender is believed to resolve a 4-sample
framebuffer, so draw both FID sets with ``--samples 4``; the default stays 1.

    python -m octfusion_amd.render --input meshes/ --out fid_images [--size 299] [--batch 8] [--samples 4]
"""
import argparse
import ctypes
import json
import math
import os
import struct
import sys
import time
import zlib

import numpy as np
import torch

from . import _lib

YFOV = math.pi / 3.0        # utils/render/render_utils.py:147
ZNEAR, ZFAR = 0.05, 100.0   # the near plane drops triangles (no clipping); depth is quantised over [ZNEAR, ZFAR]
BIG_PX = 32                 # a triangle whose clamped pixel box holds more pixels is rasterised by a wave, not a thread
WORKSPACE_BYTES = 1 << 30   # key buffer + projected vertices + large-triangle list of one chunk of views stay below
# the reference's three lights at the camera (render_utils.py:88-99, called with intensity 3.0) and the material
# believed to be pyrender's default for a mesh without one -- parameters, because that cannot be pinned here
SAMPLES = (1, 4, 16)        # samples per pixel; the positions are the library's (sample_offsets)
MATERIAL = dict(base_color=(0.3, 0.3, 0.3), metallic=0.2, roughness=0.8, directional=3.0, point=6.0, spot=3.0,
                spot_inner=math.pi / 16, spot_outer=math.pi / 6)


def fid_views():
    """[20, 3] float64 eye positions of the FID protocol: the vertices of a regular dodecahedron (circumradius
    1.07047) times 2, in four rings around z, in the order of the reference's table (utils/render/render.py:10-29)."""
    s5 = math.sqrt(5.0)
    a = math.sqrt((5.0 + s5) / 10.0)
    r = 2.0 * math.tan(math.radians(18.0))
    R = 2.0 * math.sqrt((5.0 - s5) / 10.0)
    b = a - r
    v = []
    for k in range(5):
        t = math.radians(36.0 + 72.0 * k)
        v.append((r * math.cos(t), r * math.sin(t), a))
    for k in range(10):
        t = math.radians(-36.0 + 36.0 * k)
        v.append((R * math.cos(t), R * math.sin(t), b if k % 2 == 0 else -b))
    for k in range(5):
        t = math.radians(72.0 * k)
        v.append((r * math.cos(t), r * math.sin(t), -a))
    return np.asarray(v, np.float64) * 2.0


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """[4, 4] float64 camera-to-world pose of a camera at ``eye`` looking at ``target`` (down its own -z, y up): what
    the reference's create_pose builds (render_utils.py:167-172)."""
    eye = np.asarray(eye, np.float64).reshape(3)
    f = np.asarray(target, np.float64).reshape(3) - eye
    n = math.sqrt(float(f @ f))
    if not n > 0:
        raise ValueError('look_at: eye and target coincide')
    f = f / n
    s = np.cross(f, np.asarray(up, np.float64).reshape(3))
    n = math.sqrt(float(s @ s))
    if not n > 0:
        raise ValueError('look_at: the view direction is parallel to up')
    s = s / n
    u = np.cross(s, f)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = s, u, -f, eye
    return pose


def fid_poses():
    """[20, 4, 4] poses of the 20 views."""
    return np.stack([look_at(e) for e in fid_views()])


def camera_rows(poses):
    """[V, 24] float64: per pose the view matrix (the rigid inverse: R^T, -R^T t) and the pose, 3 x 4 rows each -- the
    `cam` argument of the entry points (include/ofx.h)."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    out = np.empty((len(poses), 24), np.float64)
    for k, p in enumerate(poses):
        R, t = p[:3, :3], p[:3, 3]
        if not np.allclose(R @ R.T, np.eye(3), atol=1e-9) or not np.allclose(p[3], (0, 0, 0, 1)):
            raise ValueError('render: pose %d is not rigid (rotation + translation)' % k)
        view = np.empty((3, 4))
        view[:, :3] = R.T
        for i in range(3):
            view[i, 3] = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
        out[k, :12] = view.ravel()
        out[k, 12:] = p[:3].ravel()
    return out


def shade_params(background=1.0, **material):
    """The 13 float64 `params` of ofx_render_shade from the keyword arguments of ``render``."""
    unknown = set(material) - set(MATERIAL)
    if unknown:
        raise TypeError('render: unknown material arguments %s (known: %s)' % (sorted(unknown), sorted(MATERIAL)))
    m = dict(MATERIAL, **material)
    base = np.broadcast_to(np.asarray(m['base_color'], np.float64), (3,))
    bg = np.broadcast_to(np.asarray(background, np.float64), (3,))
    ci, co = math.cos(m['spot_inner']), math.cos(m['spot_outer'])
    scale = 1.0 / max(0.001, ci - co)
    vals = list(base) + [m['metallic'], m['roughness'], m['directional'], m['point'], m['spot'], scale, -co * scale]
    vals += list(bg)
    return [float(x) for x in vals]


def sample_offsets(samples):
    """[samples, 2] int32: the sample positions of a pixel in 1/256 pixel from its origin, read from the library
    (ofx_render_sample_offsets) so that they are the kernels' own."""
    samples = _check_samples(samples)
    xy = (ctypes.c_int32 * (2 * samples))()
    _lib.call('ofx_render_sample_offsets', samples, xy)
    return np.asarray(list(xy), np.int32).reshape(samples, 2)


def _check_samples(samples):
    if isinstance(samples, bool) or samples not in SAMPLES:
        raise ValueError('render: samples must be one of %s, got %r' % (SAMPLES, samples))
    return int(samples)


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _gather(meshes):
    """Validate on the host side of the boundary (one sync) and concatenate: (verts, faces, nv, nf)."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError('render: no meshes')
    dev = _device()
    vs, fs = [], []
    for k, m in enumerate(meshes):
        if not (isinstance(m, (tuple, list)) and len(m) == 2):
            raise ValueError('render: shape %d is not a (verts, faces) pair' % k)
        v, f = m
        v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32)))
        f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.int64)))
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError('render: shape %d must be verts [V, 3], faces [F, 3], got %s and %s'
                             % (k, tuple(v.shape), tuple(f.shape)))
        if f.shape[0] == 0:
            raise ValueError('render: shape %d has no faces' % k)
        if v.shape[0] == 0:
            raise ValueError('render: shape %d has no vertices' % k)
        vs.append(v.to(device=dev, dtype=torch.float32))
        fs.append(f.to(device=dev))
    nv = [int(v.shape[0]) for v in vs]
    nf = [int(f.shape[0]) for f in fs]
    rng = torch.stack([torch.stack([f.min(), f.max()]).to(torch.int64) for f in fs]).cpu()        # the host sync
    for k in range(len(fs)):
        if int(rng[k, 0]) < 0 or int(rng[k, 1]) >= nv[k]:
            raise ValueError('render: shape %d (verts %s, faces %s) has a face index outside [0, %d)'
                             % (k, tuple(vs[k].shape), tuple(fs[k].shape), nv[k]))
    if sum(nv) >= 2 ** 31 or sum(nf) >= 2 ** 31:
        raise ValueError('render: more than 2^31 - 1 vertices or faces in one call; pass fewer meshes')
    V = torch.cat(vs).contiguous()
    F = torch.cat([f.to(torch.int32) for f in fs]).contiguous()
    return V, F, nv, nf


def _views_per_chunk(B, n_views, size, total_verts, total_faces, samples=1):
    per_view = B * size * size * 8 * samples + total_verts * 16 + total_faces * 8
    return max(1, min(n_views, WORKSPACE_BYTES // per_view, 65535 // B))


def render(meshes, poses=None, size=299, normalize=True, background=1.0, buffers=False, big_px=None, znear=ZNEAR,
           zfar=ZFAR, samples=1, **material):
    """uint8 [B, V, size, size, 3] device tensor: every mesh of ``meshes`` -- the list ``mesh.marching_cubes`` returns,
    or ``(verts, faces)`` pairs (numpy or tensors, faces 0-based) -- seen from every pose of ``poses`` ([V, 4, 4]
    camera-to-world, rigid; None: the 20 FID views).

    normalize: first map each mesh to the unit sphere, (v - bounding-box centre) / largest distance from it, as the
    reference does.  background: grey level or rgb in [0, 1].  big_px: the pixel-box size above which a triangle takes
    the wave-per-triangle path (default BIG_PX; the images do not depend on it).  material: any of MATERIAL's keys.
    buffers=True returns ``(images, dict)`` with ``ids`` int32 [B, V, size, size] (face index, -1 background), ``depth``
    float64 (quantised window depth in [0, 1), 1.0 background), ``sxy`` int32 [V, total verts, 2] and ``vertex_depth``
    float64 [V, total verts] (the projected vertices of the concatenated meshes), ``norm`` float64 [B, 4] (centre,
    scale) and ``dropped`` int32 [B, V] (triangles dropped at the near plane or the guard band).

    samples: 1 (the pixel centre), 4 (rotated grid) or 16 samples per pixel.  With more than one, coverage and depth
    are resolved per sample, every face is shaded once per pixel at the pixel-centre ray, and the pixel is the mean of
    its samples' colours, quantised once; ``ids`` and ``depth`` gain a trailing ``samples`` axis and the dict carries
    ``sample_offsets`` int32 [samples, 2] (1/256 pixel from the pixel's origin).  Any other value raises ValueError
    before any launch.

    Views are rendered in chunks so that the key buffer, the projected vertices and the large-triangle list of one
    chunk stay under WORKSPACE_BYTES (a single view may exceed it).  One host synchronisation, for the face-index
    check; a bad mesh raises ValueError naming the shape before any launch, OfxError without a GPU."""
    samples = _check_samples(samples)
    _lib.require_device()
    size = int(size)
    if not 1 <= size <= 4096:
        raise ValueError('render: size %d outside [1, 4096]' % size)
    V, F, nv, nf = _gather(meshes)
    dev = V.device
    B = len(nv)
    if B > 65535:
        raise ValueError('render: more than 65535 meshes in one call')
    cam_all = camera_rows(fid_poses() if poses is None else poses)
    n_views = len(cam_all)
    if n_views < 1:
        raise ValueError('render: no poses')
    params = (ctypes.c_double * 13)(*shade_params(background, **material))
    big_px = BIG_PX if big_px is None else int(big_px)
    if big_px < 0:
        raise ValueError('render: big_px must be >= 0')
    tv, tf = sum(nv), sum(nf)
    voff = np.cumsum([0] + nv[:-1])
    foff = np.cumsum([0] + nf[:-1])
    offs = torch.tensor(np.concatenate([voff, nv, foff, nf]), dtype=torch.int64).to(dev)
    tan_half = math.tan(YFOV / 2.0)
    st = _lib.stream()
    chunk = _views_per_chunk(B, n_views, size, tv, tf, samples)
    ms = samples > 1                # one sample: the one-sample entry points, and buffers without the samples axis
    kshape = (size, size, samples) if ms else (size, size)
    image = torch.empty(B, n_views, size, size, 3, dtype=torch.uint8, device=dev)
    norm = torch.empty(B, 4, dtype=torch.float64, device=dev)
    keep = {k: [] for k in ('keys', 'sxy', 'vertex_depth', 'dropped')} if buffers else None
    nc = min(chunk, n_views)
    sxy = torch.empty(nc, tv, 2, dtype=torch.int32, device=dev)
    vdepth = torch.empty(nc, tv, dtype=torch.float64, device=dev)
    keys = torch.empty(B, nc, *kshape, dtype=torch.int64, device=dev)
    dropped = torch.empty(B, nc, dtype=torch.int32, device=dev)
    img = image if nc == n_views else torch.empty(B, nc, size, size, 3, dtype=torch.uint8, device=dev)
    ws = torch.empty(_lib.lib().ofx_render_raster_ws_bytes(nc, tf), dtype=torch.uint8, device=dev)
    for v0 in range(0, n_views, chunk):
        n = min(chunk, n_views - v0)
        cam = torch.from_numpy(np.ascontiguousarray(cam_all[v0:v0 + n])).to(dev)
        _lib.call('ofx_render_project', _lib.ptr(V), _lib.ptr(offs), B, tv, max(nv), _lib.ptr(cam), n, size, tan_half,
                  float(znear), float(zfar), 1 if normalize else 0, _lib.ptr(norm), _lib.ptr(sxy), _lib.ptr(vdepth), st)
        if ms:
            _lib.call('ofx_render_raster_ms', _lib.ptr(F), _lib.ptr(offs), B, tv, tf, max(nf), n, size, samples,
                      _lib.ptr(sxy), _lib.ptr(vdepth), big_px, _lib.ptr(keys), _lib.ptr(dropped), _lib.ptr(ws), st)
            _lib.call('ofx_render_shade_ms', _lib.ptr(V), _lib.ptr(F), _lib.ptr(offs), B, _lib.ptr(norm), _lib.ptr(cam),
                      n, size, samples, tan_half, _lib.ptr(keys), params, _lib.ptr(img), st)
        else:
            _lib.call('ofx_render_raster', _lib.ptr(F), _lib.ptr(offs), B, tv, tf, max(nf), n, size, _lib.ptr(sxy),
                      _lib.ptr(vdepth), big_px, _lib.ptr(keys), _lib.ptr(dropped), _lib.ptr(ws), st)
            _lib.call('ofx_render_shade', _lib.ptr(V), _lib.ptr(F), _lib.ptr(offs), B, _lib.ptr(norm), _lib.ptr(cam), n,
                      size, tan_half, _lib.ptr(keys), params, _lib.ptr(img), st)
        # a short last chunk fills the head of the flat buffers: [B, n, ...] views of them
        if img is not image:
            image[:, v0:v0 + n] = img.view(-1)[:B * n * size * size * 3].view(B, n, size, size, 3)
        if buffers:
            keep['keys'].append(keys.view(-1)[:B * n * size * size * samples].view(B, n, *kshape).clone())
            keep['sxy'].append(sxy.view(-1)[:n * tv * 2].view(n, tv, 2).clone())
            keep['vertex_depth'].append(vdepth.view(-1)[:n * tv].view(n, tv).clone())
            keep['dropped'].append(dropped.view(-1)[:B * n].view(B, n).clone())
    if not buffers:
        return image
    k = torch.cat(keep['keys'], 1)
    ids = (k & 0xFFFFFFFF).to(torch.int32)          # 0xFFFFFFFF wraps to -1: the background
    dq = (k >> 32) & 0xFFFFFFFF
    depth = torch.where(k == -1, torch.ones((), dtype=torch.float64, device=dev), dq.to(torch.float64) / 4294967296.0)
    out = dict(ids=ids, depth=depth, sxy=torch.cat(keep['sxy'], 0), vertex_depth=torch.cat(keep['vertex_depth'], 0),
               norm=norm, dropped=torch.cat(keep['dropped'], 1))
    if ms:
        out['sample_offsets'] = torch.from_numpy(sample_offsets(samples)).to(dev)
    return image, out


# ---- PNG files (zlib + struct only) --------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img):
    """The bytes of an 8-bit PNG of ``img``: uint8 [H, W, 3] (RGB) or [H, W] (grey), filter 0 on every row."""
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError('write_png: image must be uint8 [H, W, 3] or [H, W], got %s %s' % (a.dtype, a.shape))
    h, w = a.shape[:2]
    rows = np.empty((h, 1 + w * (3 if a.ndim == 3 else 1)), np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) +
            _chunk(b'IEND', b''))


def write_png(path, img):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(png_bytes(img))


def write_fid_images(root, names, images):
    """``root/view_<j>/<name>.png`` for every shape and view of ``images`` [B, V, H, W, 3] -- the layout of the
    reference's generate_image_for_fid (utils/render_utils.py:14-23), which metrics/calc_fid.py reads."""
    names = [str(n) for n in names]
    if len(names) != images.shape[0]:
        raise ValueError('write_fid_images: %d names for %d shapes' % (len(names), images.shape[0]))
    a = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    for b, name in enumerate(names):
        for j in range(a.shape[1]):
            write_png(os.path.join(root, 'view_%d' % j, name + '.png'), a[b, j])


def _inputs(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith('.obj')]
        else:
            files.append(p)
    return files


def main(argv=None):
    ap = argparse.ArgumentParser(description='render OBJ meshes from the 20 FID views into view_<j>/<name>.png')
    ap.add_argument('--input', nargs='+', required=True, help='OBJ files and / or directories of them')
    ap.add_argument('--out', required=True)
    ap.add_argument('--size', type=int, default=299)
    ap.add_argument('--batch', type=int, default=8, help='meshes per render call')
    ap.add_argument('--samples', type=int, default=1, choices=SAMPLES,
                    help='samples per pixel (4: what the reference\'s pyrender is believed to resolve)')
    args = ap.parse_args(argv)
    from . import mesh
    _lib.require_device()
    files = _inputs(args.input)
    if not files:
        raise ValueError('render: no OBJ files in %s' % args.input)
    if args.batch < 1:
        raise ValueError('render: --batch must be >= 1')
    t0 = time.perf_counter()
    dropped = 0
    for g0 in range(0, len(files), args.batch):
        group = files[g0:g0 + args.batch]
        images, buf = render([mesh.read_obj(f) for f in group], size=args.size, buffers=True, samples=args.samples)
        dropped += int(buf['dropped'].sum())
        write_fid_images(args.out, [os.path.splitext(os.path.basename(f))[0] for f in group], images)
    res = {'shapes': len(files), 'views': 20, 'size': args.size, 'samples': args.samples,
           'seconds': time.perf_counter() - t0, 'dropped_triangles': dropped}
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
