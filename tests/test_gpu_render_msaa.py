"""The multisampled renderer on the GPU (ofx_render_raster_ms / ofx_render_shade_ms through octfusion_amd.render with
samples = 4 and 16) against tests/render_ms_oracle.py: one sample through the new entries EQUAL to the old ones,
per-sample keys EQUAL to the oracle on the device's own snapped coordinates, images within one level, interior pixels
bit-equal to the one-sample render, mixed pixels at their k / S mixture, bit-equal repeats / batches / view subsets /
chunks, an analytic disc per sample plane, validation and the two command lines."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mc_oracle as M
import render_ms_oracle as MS
import render_oracle as O
from test_render_oracle import _inflate_png

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FREE_POSE = O.look_at((1.3, -0.9, 1.7), target=(0.1, 0.05, -0.1), up=(0.2, 1.0, 0.1))
CLOSE_POSE = O.look_at((0.3, 0.2, 0.93))            # inside the unit sphere's hull: triangles fall behind znear

T4 = [(96, 32), (224, 96), (32, 160), (160, 224)]
T16 = [(144, 144), (112, 80), (80, 160), (192, 112), (48, 96), (160, 208), (208, 176), (176, 48),
       (96, 224), (128, 16), (64, 32), (32, 192), (0, 128), (240, 64), (224, 240), (16, 0)]
TABLES = {1: [(128, 128)], 4: T4, 16: T16}


@functools.lru_cache(None)
def mesh(name):
    if name == 'sphere':
        return M.marching_cubes(M.sphere(24))
    if name == 'sphere32':
        return M.marching_cubes(M.sphere(32, r=0.7, center=(0.0, 0.0, 0.0)))
    if name == 'torus':
        return M.marching_cubes(M.torus(32))
    if name == 'cube':
        v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.4, 0.4) for z in (-0.3, 0.3)], np.float32)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
        return v, f
    if name == 'soup':
        rng = np.random.default_rng(11)
        v = rng.uniform(-1, 1, (360, 3)).astype(np.float32)
        f = rng.integers(0, 360, (300, 3)).astype(np.int32)          # random winding, some long slivers
        f[10] = (5, 5, 9)                                            # degenerate: a repeated vertex
        f[11] = (7, 7, 7)
        v[20] = (v[21] + v[22]) / 2                                  # nearly collinear in 3-D
        f[12] = (20, 21, 22)
        v[350:353] = [(-0.9, -0.9, 0.95), (0.9, -0.9, 0.95), (0.0, 0.9, 0.95)]      # two large triangles on the hull,
        v[353:356] = [(0.95, -0.9, -0.9), (0.95, 0.9, -0.9), (0.95, 0.0, 0.9)]      # seen from +z and from +x
        f[40] = (350, 351, 352)
        f[41] = (353, 354, 355)
        f[200] = f[40]                                               # coincident, same winding: 40 must win
        f[201] = f[41][::-1]                                         # coincident, opposite winding: 41 must win
        return v, f
    raise KeyError(name)


def _key(pose):
    return tuple(np.asarray(pose).ravel().tolist())


def poses(views):
    P = [O.look_at(e) for e in O.fid_views()]
    return np.stack([P[v] if isinstance(v, int) else np.array(v).reshape(4, 4) for v in views])


@functools.lru_cache(None)
def run(names, views, size, samples, big_px=None):
    """Device render of a batch of named meshes: (images, buffers) as numpy, computed once per argument set."""
    from octfusion_amd import render as R
    img, buf = R.render([mesh(n) for n in names], poses=poses(views), size=size, buffers=True, big_px=big_px,
                        samples=samples)
    torch.cuda.synchronize()
    return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in buf.items()}


def _slices(names):
    nv = [len(mesh(n)[0]) for n in names]
    off = np.concatenate([[0], np.cumsum(nv)])
    return [slice(int(off[k]), int(off[k + 1])) for k in range(len(names))]


@functools.lru_cache(None)
def oracle_keys(names, b, views, j, size, samples, big_px=None):
    """(ids, quantised depth, dropped) of render_ms_oracle.raster_ms on the device's own snapped vertices."""
    _, buf = run(names, views, size, samples, big_px)
    sl = _slices(names)[b]
    keys, dropped = MS.raster_ms(buf['sxy'][j, sl], buf['vertex_depth'][j, sl], mesh(names[b])[1], size, TABLES[samples])
    ids, dq = O.split_keys(keys)
    return ids, dq, dropped


def _assert_raster_equal(names, views, size, samples, big_px=None):
    _, buf = run(names, views, size, samples, big_px)
    assert buf['ids'].shape == (len(names), len(views), size, size, samples)
    assert np.array_equal(buf['sample_offsets'], np.array(TABLES[samples], np.int32))
    for b in range(len(names)):
        for j in range(len(views)):
            ids, dq, dropped = oracle_keys(names, b, views, j, size, samples, big_px)
            assert np.array_equal(buf['ids'][b, j], ids), (names[b], j)
            have_dq = np.where(ids >= 0, np.rint(buf['depth'][b, j] * 4294967296.0).astype(np.int64), 0xFFFFFFFF)
            assert np.array_equal(have_dq, dq), (names[b], j)
            assert int(buf['dropped'][b, j]) == dropped
    return buf


# ---- 1: samples = 1 through the new entry points -------------------------------------------------------------------
@pytest.mark.parametrize('names,views,size', [(('cube', 'soup'), (5, 17), 37), (('sphere',), (0,), 64)])
def test_one_sample_through_the_new_entries_equals_the_old(names, views, size):
    from octfusion_amd import _lib, render as R
    meshes = [mesh(n) for n in names]
    ref_img, buf = R.render(meshes, poses=poses(views), size=size, buffers=True)
    V, F, nv, nf = R._gather(meshes)
    dev, B, n = V.device, len(nv), len(views)
    tv, tf = sum(nv), sum(nf)
    offs = torch.tensor(np.concatenate([np.cumsum([0] + nv[:-1]), nv, np.cumsum([0] + nf[:-1]), nf]),
                        dtype=torch.int64).to(dev)
    cam = torch.from_numpy(R.camera_rows(poses(views))).to(dev)
    params = (ctypes.c_double * 13)(*R.shade_params(1.0))
    tan_half = math.tan(R.YFOV / 2.0)
    sxy, vdepth, norm = buf['sxy'].contiguous(), buf['vertex_depth'].contiguous(), buf['norm'].contiguous()
    ws = torch.empty(_lib.lib().ofx_render_raster_ws_bytes(n, tf), dtype=torch.uint8, device=dev)
    st = _lib.stream()
    out = {}
    for tag in ('old', 'new'):
        keys = torch.zeros(B, n, size, size, dtype=torch.int64, device=dev)
        dropped = torch.full((B, n), -7, dtype=torch.int32, device=dev)
        img = torch.zeros(B, n, size, size, 3, dtype=torch.uint8, device=dev)
        one = () if tag == 'old' else (1,)
        _lib.call('ofx_render_raster' + ('' if tag == 'old' else '_ms'), _lib.ptr(F), _lib.ptr(offs), B, tv, tf, max(nf),
                  n, size, *one, _lib.ptr(sxy), _lib.ptr(vdepth), R.BIG_PX, _lib.ptr(keys), _lib.ptr(dropped),
                  _lib.ptr(ws), st)
        _lib.call('ofx_render_shade' + ('' if tag == 'old' else '_ms'), _lib.ptr(V), _lib.ptr(F), _lib.ptr(offs), B,
                  _lib.ptr(norm), _lib.ptr(cam), n, size, *one, tan_half, _lib.ptr(keys), params, _lib.ptr(img), st)
        torch.cuda.synchronize()
        out[tag] = (keys, dropped, img)
    for a, b in zip(out['old'], out['new']):
        assert torch.equal(a, b)
    keys, dropped, img = out['new']
    assert torch.equal(img, ref_img) and torch.equal(dropped, buf['dropped'])
    assert torch.equal((keys & 0xFFFFFFFF).to(torch.int32), buf['ids']) and (buf['ids'] >= 0).any()
    # and render(samples=1) is the default call, shapes included
    img1, buf1 = R.render(meshes, poses=poses(views), size=size, buffers=True, samples=1)
    assert torch.equal(img1, ref_img) and sorted(buf1) == sorted(buf)
    assert all(torch.equal(buf1[k], buf[k]) for k in buf) and buf1['ids'].shape == (B, n, size, size)


# ---- 2: the key buffer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('names,views,size,samples', [
    (('sphere',), (0, 7, _key(FREE_POSE)), 37, 4),
    (('cube',), (2, 11), 64, 4),
    (('soup',), (0, 9), 64, 4),
    (('torus',), (6, _key(CLOSE_POSE)), 64, 4),
    (('sphere',), (_key(CLOSE_POSE),), 64, 4),               # the close pose drops triangles of the sphere (not of the torus)
    (('cube',), (2,), 37, 16),
    (('soup',), (9,), 37, 16),
])
def test_sample_ids_and_depth_equal_the_oracle(names, views, size, samples):
    buf = _assert_raster_equal(names, views, size, samples)
    ids = buf['ids']
    assert (ids >= 0).any()
    if names == ('soup',):
        assert not np.isin(ids, (10, 11, 200, 201)).any()   # zero area covers nothing; the lower id wins a tie
        assert np.isin(ids, (40, 41)).any()
    if names == ('sphere',) and len(views) == 1:
        assert int(buf['dropped'][0, 0]) > 0                 # counted once per triangle, not once per sample
    else:
        assert int(buf['dropped'].sum()) == 0


# ---- 3: the two raster paths ---------------------------------------------------------------------------------------
def test_both_paths_give_the_same_bits_at_four_samples():
    names, views, size = ('cube', 'sphere'), (0, 13), 64
    ref_img, ref = run(names, views, size, 4)
    for big_px in (0, 10 ** 9):                               # everything by waves / everything by threads
        img, buf = run(names, views, size, 4, big_px)
        assert np.array_equal(img, ref_img)
        for k in ('ids', 'depth', 'dropped', 'sxy'):
            assert np.array_equal(buf[k], ref[k]), (k, big_px)
    _assert_raster_equal(names, views, size, 4, 0)


# ---- 4: screen-filling triangles -----------------------------------------------------------------------------------
def test_screen_filling_triangles_are_bounded_by_the_screen_at_four_samples():
    """The one-sample test's scene: twelve triangles far larger than the screen (a 40 x 32 x 24 box whose front face
    is one unit from the eye).  Every loop runs over the clamped box; the keys equal the oracle's."""
    from octfusion_amd import render as R
    v, f = mesh('cube')
    pose = O.look_at((0.5, 0.3, 13.0), target=(0.5, 0.3, 0.0))
    big = (v * 40.0).astype(np.float32)
    want = None
    for big_px in (None, 2 ** 40):
        img, buf = R.render([(big, f)], poses=pose[None], size=96, normalize=False, buffers=True, big_px=big_px,
                            samples=4)
        if want is None:
            keys, dropped = MS.raster_ms(buf['sxy'][0].cpu().numpy(), buf['vertex_depth'][0].cpu().numpy(), f, 96, T4)
            want = O.split_keys(keys)[0]
        assert np.array_equal(buf['ids'][0, 0].cpu().numpy(), want)
        assert int(buf['dropped'][0, 0]) == dropped == 0
    assert (buf['ids'] >= 0).all()                            # the front face fills the screen


# ---- 5: shading ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('names,views,size,samples', [
    (('sphere',), (0, 12), 64, 4),
    (('cube', 'soup'), (5, 17), 37, 4),
    (('cube',), (5,), 37, 16),
])
def test_images_within_one_level_of_the_oracle(names, views, size, samples):
    img, buf = run(names, views, size, samples)
    ps = poses(views)
    mixed = 0
    for b, name in enumerate(names):
        v, f = mesh(name)
        for j in range(len(views)):
            ids = buf['ids'][b, j]
            want = MS.shade_ms(v, f, ids, ps[j], size, buf['norm'][b, :3], buf['norm'][b, 3])
            assert np.abs(img[b, j].astype(int) - want.astype(int)).max() <= 1
            bg = (ids < 0).all(2)
            assert bg.any() and (img[b, j][bg] == 255).all()            # background only: exactly the background
            lit = img[b, j][~bg]
            assert lit.size and (lit[:, 0] == lit[:, 1]).all()          # grey material: r = g = b
            distinct = np.array([[len(set(p.tolist())) for p in row] for row in ids])
            mixed += int((distinct > 1).sum())
    assert mixed > 0                                                    # the resolve had something to average


# ---- 6, 7: against the one-sample render ---------------------------------------------------------------------------
@pytest.mark.parametrize('samples', [4, 16])
def test_interior_pixels_are_bit_equal_to_the_one_sample_render(samples):
    names, views, size = ('cube',), (2, 11), 64
    img1, buf1 = run(names, views, size, 1)
    img, buf = run(names, views, size, samples)
    ids1, ids = buf1['ids'], buf['ids']
    interior = (ids1 >= 0) & (ids == ids1[..., None]).all(-1)
    covered = (ids >= 0).any(-1)
    assert interior.sum() > 0.5 * covered.sum() > 0          # a condition on the scene: the set is not empty
    assert np.array_equal(img[interior], img1[interior])


@pytest.mark.parametrize('samples', [4, 16])
def test_anti_aliasing_happened(samples):
    """Pixels whose samples are split between the background and ONE face: the level is the k / S mixture of that
    face's colour at the pixel and the background.  The face's colour is the one-sample image's where the one-sample
    render has that face at the pixel (one more rounding, <= k / (2 S) level), the oracle's centre-ray colour
    elsewhere (the pixel centre is outside the face)."""
    names, views, size = ('cube',), (2, 11), 64
    img1, buf1 = run(names, views, size, 1)
    img, buf = run(names, views, size, samples)
    v, f = mesh('cube')
    ps = poses(views)
    strictly_between = 0
    checked = 0
    for j in range(len(views)):
        ids, ids1 = buf['ids'][0, j], buf1['ids'][0, j]
        face = ids.max(-1)                                    # the face, if there is only one
        k = (ids >= 0).sum(-1)
        one_face = ((ids == face[..., None]) | (ids < 0)).all(-1)
        split = one_face & (k > 0) & (k < samples)
        assert split.any()
        col = MS.face_colours(v, f, np.where(split, face, -1), ps[j], size, buf['norm'][0, :3], buf['norm'][0, 3])
        c = np.clip(col[0], 0.0, 1.0) * 255.0                 # grey: one channel
        same = split & (ids1 == face)
        c = np.where(same, img1[0, j, :, :, 0].astype(np.float64), c)
        want = (k * c + (samples - k) * 255.0) / samples
        for ch in range(3):
            assert (np.abs(img[0, j, :, :, ch].astype(np.float64) - want)[split] <= 1.0 + 1e-9).all()
        lvl = img[0, j, :, :, 0].astype(np.float64)
        strictly_between += int((split & (lvl > np.minimum(c, 255.0)) & (lvl < np.maximum(c, 255.0))).sum())
        checked += int(split.sum())
        assert same.any()
    assert strictly_between > 0 and checked >= 2 * len(views)


# ---- 8: invariance -------------------------------------------------------------------------------------------------
def test_runs_batches_view_subsets_and_chunks_are_bit_equal_at_four_samples():
    from octfusion_amd import render as R
    size = 64
    meshes = [mesh('cube'), mesh('torus'), mesh('sphere')]
    full, fb = R.render(meshes, size=size, buffers=True, samples=4)           # the 20 views
    again, ab = R.render(meshes, size=size, buffers=True, samples=4)
    assert full.shape == (3, 20, size, size, 3) and full.dtype == torch.uint8
    assert fb['ids'].shape == fb['depth'].shape == (3, 20, size, size, 4)
    assert torch.equal(full, again) and all(torch.equal(fb[k], ab[k]) for k in fb)
    assert torch.equal(R.render(meshes, size=size, samples=4), full)          # without the buffers
    alone, sb = R.render([meshes[1]], size=size, buffers=True, samples=4)     # the middle of the batch, alone
    assert torch.equal(alone[0], full[1]) and torch.equal(sb['ids'][0], fb['ids'][1])
    assert torch.equal(sb['depth'][0], fb['depth'][1])
    one, ob = R.render(meshes, poses=poses([13]), size=size, buffers=True, samples=4)     # one view, alone
    assert torch.equal(one[:, 0], full[:, 13]) and torch.equal(ob['ids'][:, 0], fb['ids'][:, 13])
    # chunking over views does not show: room for 7 views by the per-view formula with its samples term
    tv, tf = fb['sxy'].shape[1], sum(len(m[1]) for m in meshes)
    per_view = 3 * size * size * 8 * 4 + tv * 16 + tf * 8
    saved = R.WORKSPACE_BYTES
    try:
        R.WORKSPACE_BYTES = 7 * per_view
        assert R._views_per_chunk(3, 20, size, tv, tf, 4) == 7 and R._views_per_chunk(3, 20, size, tv, tf) > 7
        chunked, cb = R.render(meshes, size=size, buffers=True, samples=4)
    finally:
        R.WORKSPACE_BYTES = saved
    assert torch.equal(chunked, full) and all(torch.equal(fb[k], cb[k]) for k in fb)
    # and it differs from the one-sample render only where samples disagree
    base = R.render(meshes, size=size)
    same = (fb['ids'] == fb['ids'][..., :1]).all(-1)
    assert not torch.equal(base, full) and same.any() and not same.all()


# ---- 9: analytic ---------------------------------------------------------------------------------------------------
def test_unit_sphere_covers_the_analytic_disc_in_every_sample_plane():
    """The one-sample test's bound (tests/test_gpu_render.py), per sample plane: the silhouette lies between the
    discs of radius R(rho) and R(1) about the image centre, and the lattice-point lemma -- the number of lattice
    points in a disc of radius R is within 2 pi R of its area -- holds for any shifted lattice, so for the samples
    (i + ox / 256, j + oy / 256): |covered - pi R(1)^2| <= pi (R(1)^2 - R(rho)^2) + 2 pi R(1)."""
    size, name = 96, 'sphere32'
    _, buf = run((name,), (0,), size, 4)
    v, f = mesh(name)
    c, s = O.normalization(v)
    p = (v.astype(np.float64) - c) / s
    a, b_, c_ = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = np.cross(b_ - a, c_ - a)
    rho = float(np.abs(np.einsum('ij,ij->i', n, a) / np.linalg.norm(n, axis=1)).min())
    d = float(np.linalg.norm(O.fid_views()[0]))

    def radius(r):
        return size / 2 * math.tan(math.asin(r / d)) / math.tan(math.pi / 6)
    R1, Rr = radius(1.0), radius(rho)
    assert 0.99 < rho <= 1.0 and abs(R1 - 43.9) < 0.1
    bound = math.pi * (R1 * R1 - Rr * Rr) + 2 * math.pi * R1
    for k, (ox, oy) in enumerate(T4):
        covered = buf['ids'][0, 0, :, :, k] >= 0
        assert abs(int(covered.sum()) - math.pi * R1 * R1) <= bound
        ys, xs = np.nonzero(covered)
        rr = np.hypot(xs + ox / 256 - size / 2, ys + oy / 256 - size / 2)
        assert rr.max() <= R1 + 1 / 256 + 1e-9                # nothing outside the unit ball's disc
    planes = (buf['ids'][0, 0] >= 0).sum((0, 1))
    assert len(set(planes.tolist())) > 1                      # the planes are different lattices


# ---- 10: validation ------------------------------------------------------------------------------------------------
def test_bad_sample_counts_are_refused(monkeypatch):
    from octfusion_amd import _lib, render as R
    v, f = mesh('cube')

    def no_gather(meshes):
        raise AssertionError('render went on to _gather')
    with monkeypatch.context() as mp:
        mp.setattr(R, '_gather', no_gather)
        for s in (0, 2, 3, 8, 32):
            with pytest.raises(ValueError, match='samples'):
                R.render([(v, f)], size=16, samples=s)
    with pytest.raises(ValueError):
        R.sample_offsets(2)
    L = _lib.lib()
    for S in (1, 4, 16):
        xy = (ctypes.c_int32 * (2 * S))()
        assert L.ofx_render_sample_offsets(S, xy) == 0
        assert [tuple(xy[2 * k:2 * k + 2]) for k in range(S)] == TABLES[S]
        assert R.sample_offsets(S).tolist() == [list(t) for t in TABLES[S]]
    xy = (ctypes.c_int32 * 64)(*([-5] * 64))
    assert L.ofx_render_sample_offsets(2, xy) == -1 and L.ofx_render_sample_offsets(4, None) == -1
    assert list(xy) == [-5] * 64
    # the launching entries: everything valid but the sample count -- refused, nothing written
    _, buf = R.render([(v, f)], poses=poses([0]), size=16, buffers=True)
    dev = buf['sxy'].device
    V, F, nv, nf = R._gather([(v, f)])
    offs = torch.tensor([0, nv[0], 0, nf[0]], dtype=torch.int64, device=dev)
    cam = torch.from_numpy(R.camera_rows(poses([0]))).to(dev)
    keys = torch.full((16, 16, 16), 5, dtype=torch.int64, device=dev)
    dropped = torch.full((1,), 5, dtype=torch.int32, device=dev)
    img = torch.full((16, 16, 3), 5, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.ofx_render_raster_ws_bytes(1, nf[0]), dtype=torch.uint8, device=dev)
    params = (ctypes.c_double * 13)(*R.shade_params(1.0))
    st = _lib.stream()
    rc = L.ofx_render_raster_ms(_lib.ptr(F), _lib.ptr(offs), 1, nv[0], nf[0], nf[0], 1, 16, 2, _lib.ptr(buf['sxy']),
                                _lib.ptr(buf['vertex_depth']), 32, _lib.ptr(keys), _lib.ptr(dropped), _lib.ptr(ws), st)
    assert rc == -1
    rc = L.ofx_render_shade_ms(_lib.ptr(V), _lib.ptr(F), _lib.ptr(offs), 1, _lib.ptr(buf['norm']), _lib.ptr(cam), 1, 16,
                               2, math.tan(R.YFOV / 2.0), _lib.ptr(keys), params, _lib.ptr(img), st)
    assert rc == -1
    torch.cuda.synchronize()
    assert (keys == 5).all() and (dropped == 5).all() and (img == 5).all()


# ---- 11: end to end ------------------------------------------------------------------------------------------------
def test_cli_takes_samples(tmp_path, capsys):
    from octfusion_amd import mesh as PM, render as R
    src = tmp_path / 'objs'
    for name in ('cube', 'sphere'):
        PM.write_obj(str(src / (name + '.obj')), *mesh(name))
    out = tmp_path / 'fid'
    res = R.main(['--input', str(src), '--out', str(out), '--size', '37', '--batch', '2', '--samples', '4'])
    rec = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert rec['shapes'] == 2 and rec['samples'] == 4 and res['samples'] == 4
    objs = [PM.read_obj(str(src / 'cube.obj')), PM.read_obj(str(src / 'sphere.obj'))]
    want = R.render(objs, size=37, samples=4).cpu().numpy()
    assert not np.array_equal(want, R.render(objs, size=37).cpu().numpy())
    for j in range(20):
        for b, name in enumerate(('cube', 'sphere')):
            got = _inflate_png(open(out / ('view_%d' % j) / (name + '.png'), 'rb').read())
            assert np.array_equal(got, want[b, j])
    with pytest.raises(SystemExit):
        R.main(['--input', str(src), '--out', str(out), '--samples', '3'])


def test_generate_cli_takes_view_samples(tmp_path, capsys):
    from octfusion_amd import configs, generate as G, mesh as PM, render as R
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    PM.MESH_SCALES['tiny_uncond'] = PM.MESH_SCALES['snet_uncond']
    out_dir = str(tmp_path / 'gen')
    res = G.main(['--config', 'tiny_uncond', '--shapes', '2', '--steps', '2', '--batch', '2', '--sdf-resolution', '64',
                  '--seed', '5', '--mesh', '--views', '--view-size', '64', '--view-samples', '4', '--out', out_dir])
    written = 0
    for i in res['rank0_indices']:
        obj = os.path.join(out_dir, '%d.obj' % i)
        pngs = [os.path.join(out_dir, 'fid_images', 'view_%d' % j, '%d.png' % i) for j in range(20)]
        assert all(os.path.exists(p) == os.path.exists(obj) for p in pngs)
        if not os.path.exists(obj):
            continue
        # the OBJ round trip is exact, so rendering the written mesh gives the written images
        want = R.render([PM.read_obj(obj)], size=64, samples=4).cpu().numpy()
        one = R.render([PM.read_obj(obj)], size=64).cpu().numpy()
        assert want.shape == (1, 20, 64, 64, 3) and not np.array_equal(want, one)
        for j in (0, 13):
            assert np.array_equal(_inflate_png(open(pngs[j], 'rb').read()), want[0, j])
        written += 1
    assert written > 0
