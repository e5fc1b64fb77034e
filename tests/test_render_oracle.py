"""CPU checks of the renderer's oracle (tests/render_oracle.py) and of the host side of octfusion_amd.render: the
integer rasteriser against exact rational arithmetic, the view table, the PNG writer and the C-ABI exports."""
import json
import os
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest

import render_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 8


def _brute_coverage(tri, size):
    """Top-left rule by its definition: the pixel centre moved by (+eps, +eps^2) lies strictly inside the triangle.
    Coordinates are multiples of 1/256 pixel and edge functions multiples of 2^-16, so eps = 2^-40 decides every
    on-edge case without changing any off-edge one."""
    eps = Fraction(1, 2 ** 40)
    (ax, ay), (bx, by), (cx, cy) = [(Fraction(int(x), 256), Fraction(int(y), 256)) for x, y in tri]
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    out = np.zeros((size, size), bool)
    if area == 0:
        return out
    for j in range(size):
        for i in range(size):
            px, py = Fraction(2 * i + 1, 2) + eps, Fraction(2 * j + 1, 2) + eps * eps
            e = [(bx - ax) * (py - ay) - (by - ay) * (px - ax), (cx - bx) * (py - by) - (cy - by) * (px - bx),
                 (ax - cx) * (py - cy) - (ay - cy) * (px - cx)]
            out[j, i] = all(x * area > 0 for x in e)
    return out


def _brute_keys(sxy, depth, faces, size):
    """Visibility with exact rational depth: per pixel the covering triangle of least quantised depth, lowest id."""
    keys = np.full((size, size), O.EMPTY, np.uint64)
    for f, (ia, ib, ic) in enumerate(faces):
        tri = [tuple(int(t) for t in sxy[k]) for k in (ia, ib, ic)]
        cov = _brute_coverage(tri, size)
        (ax, ay), (bx, by), (cx, cy) = tri
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        for j, i in zip(*np.nonzero(cov)):
            px, py = 256 * int(i) + 128, 256 * int(j) + 128
            wa = (cx - bx) * (py - by) - (cy - by) * (px - bx)
            wb = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
            wc = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            d = (wa * Fraction(depth[ia]) + wb * Fraction(depth[ib]) + wc * Fraction(depth[ic])) / area
            q = min(max(int(d * 2 ** 32), 0), 2 ** 32 - 1)
            keys[j, i] = min(int(keys[j, i]), (q << 32) | f)
    return keys


P = 256
# depths are dyadic with few bits, so the float64 interpolation is exact and must agree with the rational one
CASES = {
    'quad_shared_diagonal': ([(1 * P, 1 * P), (6 * P, 1 * P), (6 * P, 6 * P), (1 * P, 6 * P)],
                             [(0, 1, 2), (0, 2, 3)], [0.25, 0.25, 0.25, 0.25]),
    'fan_opposite_windings': ([(4 * P, 4 * P), (0, P), (7 * P + 128, 300), (8 * P, 7 * P), (300, 8 * P - 1)],
                              [(0, 1, 2), (0, 3, 2), (0, 3, 4), (0, 1, 4)], [0.5, 0.25, 0.75, 0.5, 0.125]),
    'vertex_on_pixel_centre': ([(3 * P + 128, 2 * P + 128), (6 * P + 128, 2 * P + 128), (3 * P + 128, 5 * P + 128),
                                (6 * P + 128, 5 * P + 128)], [(0, 1, 2), (2, 1, 3)], [0.5, 0.5, 0.5, 0.5]),
    'zero_area': ([(P, P), (4 * P, 4 * P), (7 * P, 7 * P), (2 * P, 5 * P)],
                  [(0, 1, 2), (0, 0, 3), (3, 3, 3), (0, 3, 2)], [0.5, 0.5, 0.5, 0.25]),
    'coincident': ([(0, 0), (8 * P, 0), (0, 8 * P), (0, 0), (8 * P, 0), (0, 8 * P)],
                   [(3, 4, 5), (0, 1, 2), (2, 1, 0)], [0.5, 0.25, 0.75, 0.5, 0.25, 0.75]),
    'off_screen_and_slivers': ([(-3 * P, -2 * P), (20 * P, 3 * P), (2 * P, 30 * P), (130, 128), (131, 4 * P), (129, 7 * P)],
                               [(0, 1, 2), (3, 4, 5), (5, 4, 3)], [0.125, 0.5, 0.875, 0.0625, 0.0625, 0.0625]),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_rasteriser_against_exact_rationals(name):
    pts, faces, depth = CASES[name]
    sxy = np.array(pts, np.int64)
    keys, dropped = O.raster(sxy, np.array(depth), faces, SIZE)
    assert dropped == 0
    want = _brute_keys(sxy, depth, faces, SIZE)
    assert np.array_equal(keys, want)
    for f, tri in enumerate(faces):
        assert np.array_equal(O.coverage([pts[k] for k in tri], SIZE), _brute_coverage([pts[k] for k in tri], SIZE)), f


def test_zero_area_covers_nothing_and_lowest_id_wins():
    pts, faces, depth = CASES['zero_area']
    for tri in faces[:3]:
        assert not O.coverage([pts[k] for k in tri], SIZE).any()
    pts, faces, depth = CASES['coincident']
    ids, _ = O.split_keys(O.raster(np.array(pts), np.array(depth), faces, SIZE)[0])
    assert set(np.unique(ids)) == {-1, 0}            # three coincident triangles, either winding: the lowest id


def test_shared_edges_cover_every_pixel_exactly_once():
    """A random fan around an interior vertex, random windings, vertices on arbitrary sub-pixel positions: the
    triangles tile the polygon, so the per-triangle coverages are disjoint and their union is the polygon's."""
    rng = np.random.default_rng(3)
    for trial in range(20):
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        if np.diff(np.concatenate([ang, ang[:1] + 2 * np.pi])).max() >= np.pi:
            continue                                  # the centre must see every rim edge from the inside
        rad = rng.uniform(1.5, 3.9, n)
        c = np.array([4 * P, 4 * P]) + rng.integers(-200, 200, 2)
        rim = np.rint(np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None] * P).astype(np.int64) + c
        total = np.zeros((SIZE, SIZE), int)
        for k in range(n):
            tri = [tuple(c), tuple(rim[k]), tuple(rim[(k + 1) % n])]
            if rng.random() < 0.5:
                tri = tri[::-1]
            total += O.coverage(tri, SIZE)
        assert total.max() <= 1
        poly = np.zeros((SIZE, SIZE), bool)
        for k in range(n):
            poly |= _brute_coverage([tuple(c), tuple(rim[k]), tuple(rim[(k + 1) % n])], SIZE)
        assert np.array_equal(total.astype(bool), poly)


def test_dropped_vertices_drop_their_triangles():
    sxy = np.array([(P, P), (6 * P, P), (P, 6 * P), (O.DROPPED, 0)], np.int64)
    keys, dropped = O.raster(sxy, np.full(4, 0.5), [(0, 1, 2), (0, 1, 3), (3, 3, 3)], SIZE)
    assert dropped == 2 and set(np.unique(O.split_keys(keys)[0])) == {-1, 0}
    # projection: behind the near plane, NaN and the guard band all fall into the drop
    pose = O.look_at((0.0, 0.0, 2.0))
    v = np.array([[0, 0, 0], [0, 0, 1.96], [0, 0, 3], [np.nan, 0, 0], [1e6, 0, 1.9], [0, np.inf, 0]], np.float32)
    s, d, _, _ = O.project(v, pose, 64, np.zeros(3), 1.0)
    assert (s[:, 0] == O.DROPPED).tolist() == [False, True, True, True, True, True]
    assert tuple(s[0]) == (64 * 128, 64 * 128) and 0.0 < d[0] < 1.0 and (d[1:] == 0).all()


def test_fid_views_match_the_reference_table():
    from octfusion_amd import render as R
    tab = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'fid_views.json')))
    want = np.array(tab['views'], np.float64)
    have = R.fid_views()
    assert have.shape == (20, 3) and have.dtype == np.float64
    assert np.abs(have / tab['scale'] - want).max() < 5e-5          # the table's printed precision
    norms = np.linalg.norm(have, axis=1)
    assert np.ptp(norms) < 1e-12 and abs(norms[0] - 2 * 1.07047) < 1e-4
    assert np.abs(have - O.fid_views()).max() < 1e-12
    # the unit sphere stays inside the 60 degree frustum from every view, so the protocol never needs near clipping
    assert np.degrees(np.arcsin(1.0 / norms[0])) < 30.0
    for e in have:
        pose = R.look_at(e)
        assert np.allclose(pose, O.look_at(e), atol=1e-12)
        Rm = pose[:3, :3]
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.linalg.det(Rm) > 0
        assert np.allclose(pose[:3, 3], e) and np.allclose(-Rm[:, 2], -e / np.linalg.norm(e))
    cam = R.camera_rows(R.fid_poses())
    assert cam.shape == (20, 24)
    assert np.allclose(cam[7, :12].reshape(3, 4), np.linalg.inv(R.look_at(have[7]))[:3], atol=1e-12)
    assert np.array_equal(cam[7, :12].reshape(3, 4), O.view_matrix(R.look_at(have[7])))
    with pytest.raises(ValueError):
        R.camera_rows([np.diag([2.0, 1, 1, 1])])
    assert R.shade_params(0.5, roughness=0.5)[:5] == [0.3, 0.3, 0.3, 0.2, 0.5]
    with pytest.raises(TypeError):
        R.shade_params(gloss=1.0)


def _inflate_png(data):
    """Decode an 8-bit grey / RGB PNG with filter type 0 rows: chunk walk, CRCs, zlib."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, bits, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (bits, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    raw = zlib.decompress(b''.join(b for t, b in chunks if t == b'IDAT'))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


def test_write_png_round_trip(tmp_path):
    from octfusion_amd import render as R
    rng = np.random.default_rng(0)
    for shape in ((5, 7, 3), (1, 1, 3), (9, 4), (299, 299, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / 'sub' / ('%d.png' % len(shape)))
        R.write_png(path, img)
        assert np.array_equal(_inflate_png(open(path, 'rb').read()), img)
    with pytest.raises(ValueError):
        R.png_bytes(np.zeros((4, 4, 3), np.float32))
    images = rng.integers(0, 256, (2, 3, 6, 6, 3), dtype=np.uint8)
    R.write_fid_images(str(tmp_path / 'fid'), ['a', 7], images)
    for b, name in enumerate(('a', '7')):
        for j in range(3):
            got = _inflate_png(open(str(tmp_path / 'fid' / ('view_%d' % j) / (name + '.png')), 'rb').read())
            assert np.array_equal(got, images[b, j])
    with pytest.raises(ValueError):
        R.write_fid_images(str(tmp_path / 'fid'), ['a'], images)


def test_render_exports_are_bound():
    from octfusion_amd import _lib, build
    assert 'ofx_render.hip' in build.SOURCES
    for name in ('ofx_render_project', 'ofx_render_raster', 'ofx_render_raster_ws_bytes', 'ofx_render_shade'):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    assert L.ofx_render_raster_ws_bytes(0, 5) == 0 and L.ofx_render_raster_ws_bytes(3, 100) >= 3 * 100 * 8
    # bad arguments are refused before anything is launched (so this needs no device)
    assert L.ofx_render_project(None, None, 1, 1, 1, None, 1, 8, 0.5, 0.05, 100.0, 1, None, None, None, None) == -1
    assert L.ofx_render_raster(None, None, 1, 1, 1, 1, 1, 8, None, None, 0, None, None, None, None) == -1
    assert L.ofx_render_shade(None, None, None, 1, None, None, 1, 8, 0.5, None, None, None, None) == -1


def test_oracle_shading_is_two_sided_and_bounded():
    """A square facing the camera: both windings shade alike, the centre is brighter than the corner (the point and
    spot lights fall off), and the closed form at the centre pixel of an odd image is the one of DESIGN.md 4.14."""
    size = 9
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    pose = O.look_at((0.0, 0.0, 2.0))
    imgs = []
    for faces in ([(0, 1, 2), (0, 2, 3)], [(2, 1, 0), (3, 2, 0)]):
        s, d, _, _ = O.project(v, pose, size, np.zeros(3), 1.0)
        ids, _ = O.split_keys(O.raster(s, d, faces, size)[0])
        imgs.append(O.shade(v, faces, ids, pose, size, np.zeros(3), 1.0))
    assert np.array_equal(imgs[0], imgs[1])
    img = imgs[0]
    assert (img[0, 0] == 255).all()                   # background: the square spans +-1 of +-2 tan 30
    c = img[size // 2, size // 2].astype(int)
    assert c[0] == c[1] == c[2] and c[0] > img[2, 2, 0] > 0
    # centre pixel: N = V = L for all three lights, distance 2, spot fully open
    a2 = 0.8 ** 4
    f0 = 0.04 * 0.8 + 0.3 * 0.2
    brdf = (1 - f0) * 0.3 * 0.8 / np.pi + f0 * (a2 / (np.pi * a2 * a2)) / 4.0
    assert abs(c[0] - 255 * min(1.0, (3.0 + 6.0 / 4 + 3.0 / 4) * brdf)) <= 0.5 + 1e-9
