"""The renderer on the GPU (csrc/ofx_render.hip through octfusion_amd.render) against tests/render_oracle.py:
projection within one sub-pixel unit, the key buffer EQUAL to the integer oracle run on the device's own snapped
coordinates, shading within one level, bit-equal repeats / batches / view subsets, an analytic disc, and the two
command lines."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mc_oracle as M
import render_oracle as O
from test_render_oracle import _inflate_png

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FREE_POSE = O.look_at((1.3, -0.9, 1.7), target=(0.1, 0.05, -0.1), up=(0.2, 1.0, 0.1))
CLOSE_POSE = O.look_at((0.3, 0.2, 0.93))            # inside the unit sphere's hull: triangles fall behind znear
CLOSE_TORUS = O.look_at((0.72, 0.0, 0.2), target=(-0.7, 0.1, 0.0))    # grazing the normalised torus's tube


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


def poses(views):
    P = [O.look_at(e) for e in O.fid_views()]
    return np.stack([P[v] if isinstance(v, int) else v for v in views])


@functools.lru_cache(None)
def run(names, views, size, big_px=None, normalize=True):
    """Device render of a batch of named meshes: (images, buffers) as numpy, computed once per argument set."""
    from octfusion_amd import render as R
    ps = None if views is None else poses([v if isinstance(v, int) else np.array(v).reshape(4, 4) for v in views])
    img, buf = R.render([mesh(n) for n in names], poses=ps, size=size, buffers=True, big_px=big_px, normalize=normalize)
    torch.cuda.synchronize()
    return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in buf.items()}


def _key(pose):
    return tuple(np.asarray(pose).ravel().tolist())


def _slices(names):
    nv = [len(mesh(n)[0]) for n in names]
    off = np.concatenate([[0], np.cumsum(nv)])
    return [slice(int(off[k]), int(off[k + 1])) for k in range(len(names))]


def _oracle_ids(names, b, buf, j, size):
    """The oracle's (ids, quantised depth, dropped) from the device's own snapped vertices of mesh b, view slot j."""
    sl = _slices(names)[b]
    keys, dropped = O.raster(buf['sxy'][j, sl], buf['vertex_depth'][j, sl], mesh(names[b])[1], size)
    ids, dq = O.split_keys(keys)
    return ids, dq, dropped


def _assert_raster_equal(names, views, size, big_px=None):
    _, buf = run(names, views, size, big_px)
    for b in range(len(names)):
        for j in range(len(views)):
            ids, dq, dropped = _oracle_ids(names, b, buf, j, size)
            assert np.array_equal(buf['ids'][b, j], ids), (names[b], views[j] if isinstance(views[j], int) else 'free')
            have_dq = np.where(ids >= 0, np.rint(buf['depth'][b, j] * 4294967296.0).astype(np.int64), 0xFFFFFFFF)
            assert np.array_equal(have_dq, dq)
            assert int(buf['dropped'][b, j]) == dropped
    return buf


# ---- projection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [96, 299])
def test_projection_within_one_unit_of_float64(size):
    names = ('sphere', 'soup')
    views = tuple(range(20)) + (_key(FREE_POSE),)
    _, buf = run(names, views, size)
    for b, sl in enumerate(_slices(names)):
        c, s = O.normalization(mesh(names[b])[0])
        assert np.abs(buf['norm'][b, :3] - c).max() <= 1e-6 * np.abs(c).max() + 1e-12
        assert abs(buf['norm'][b, 3] - s) <= 1e-6 * s
        for j, pose in enumerate(poses([v if isinstance(v, int) else np.array(v).reshape(4, 4) for v in views])):
            want, depth, _, _ = O.project(mesh(names[b])[0], pose, size, c, s)
            assert (want[:, 0] != O.DROPPED).all()
            assert np.abs(buf['sxy'][j, sl].astype(np.int64) - want).max() <= 1
            assert np.abs(buf['vertex_depth'][j, sl] - depth).max() <= 1e-12
    assert (buf['dropped'] == 0).all()


# ---- raster --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('names,views,size', [
    (('sphere',), (0, 7, 13, _key(FREE_POSE)), 37),          # sub-pixel to few-pixel triangles
    (('sphere',), (4, 18), 64),
    (('cube',), tuple(range(20)) + (_key(FREE_POSE),), 37),  # twelve large triangles
    (('cube',), (2, 11), 96),
    (('soup',), (0, 9, 16, _key(FREE_POSE)), 64),            # random winding, degenerate and coincident triangles
    (('torus',), (6, _key(CLOSE_POSE)), 64),
])
def test_ids_equal_the_integer_oracle(names, views, size):
    buf = _assert_raster_equal(names, views, size)
    assert (buf['ids'] >= 0).any()
    if names == ('soup',):
        ids = buf['ids']
        assert not np.isin(ids, (10, 11, 200, 201)).any()   # zero area covers nothing; the lower id wins a tie
        assert np.isin(ids, (40, 41)).any()


def test_close_pose_drops_triangles_like_the_oracle():
    for name, pose in (('sphere', CLOSE_POSE), ('torus', CLOSE_TORUS)):
        buf = _assert_raster_equal((name,), (_key(pose),), 64)
        assert int(buf['dropped'][0, 0]) > 0 and (buf['ids'] >= 0).any()
        c, s = O.normalization(mesh(name)[0])
        want, _, _, _ = O.project(mesh(name)[0], pose, 64, c, s)
        assert np.array_equal(buf['sxy'][0, :, 0] == O.DROPPED, want[:, 0] == O.DROPPED)


def test_both_paths_give_the_same_bits():
    names, views, size = ('sphere', 'cube', 'soup'), (0, 9, _key(CLOSE_POSE)), 64
    ref_img, ref = run(names, views, size)
    for big_px in (0, 2 ** 40):                               # everything by waves / everything by threads
        img, buf = run(names, views, size, big_px)
        assert np.array_equal(img, ref_img)
        for k in ('ids', 'depth', 'dropped', 'sxy'):
            assert np.array_equal(buf[k], ref[k]), (k, big_px)
    _assert_raster_equal(names, views, size, 0)


def test_the_switch_between_the_paths():
    """One triangle whose clamped pixel box holds n pixels: big_px = n keeps it on the thread path (box == big_px),
    big_px = n - 1 sends it to the wave path (box == big_px + 1); same keys, equal to the oracle's."""
    from octfusion_amd import render as R
    v = np.array([[-0.8, -0.5, 0.1], [0.9, -0.2, -0.3], [0.1, 0.7, 0.2]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    size = 37
    pose = poses([3])
    _, base = R.render([(v, f)], poses=pose, size=size, buffers=True)
    s = base['sxy'][0].cpu().numpy().astype(np.int64)
    x0, x1 = max((s[:, 0].min() - 128 + 255) // 256, 0), min((s[:, 0].max() - 128) // 256, size - 1)
    y0, y1 = max((s[:, 1].min() - 128 + 255) // 256, 0), min((s[:, 1].max() - 128) // 256, size - 1)
    n = int((x1 - x0 + 1) * (y1 - y0 + 1))
    assert n > 64
    keys, _ = O.raster(s, base['vertex_depth'][0].cpu().numpy(), f, size)
    want_ids, _ = O.split_keys(keys)
    assert (want_ids == 0).sum() > 30
    for big_px in (n, n - 1, n + 1, 0):
        img, buf = R.render([(v, f)], poses=pose, size=size, buffers=True, big_px=big_px)
        assert np.array_equal(buf['ids'][0, 0].cpu().numpy(), want_ids), big_px
        assert torch.equal(buf['depth'], base['depth'])


def test_screen_filling_triangles_are_bounded_by_the_screen():
    """Twelve triangles far larger than the screen (a 40 x 32 x 24 box whose front face is one unit from the eye: its
    corners project 34 half-screens out, inside the guard band): every loop runs over the clamped box, and the
    buffers equal the oracle's."""
    v, f = mesh('cube')
    from octfusion_amd import render as R
    pose = O.look_at((0.5, 0.3, 13.0), target=(0.5, 0.3, 0.0))
    big = (v * 40.0).astype(np.float32)
    for big_px in (None, 2 ** 40):
        img, buf = R.render([(big, f)], poses=pose[None], size=96, normalize=False, buffers=True, big_px=big_px)
        keys, dropped = O.raster(buf['sxy'][0].cpu().numpy(), buf['vertex_depth'][0].cpu().numpy(), f, 96)
        assert np.array_equal(buf['ids'][0, 0].cpu().numpy(), O.split_keys(keys)[0])
        assert int(buf['dropped'][0, 0]) == dropped
    assert int(buf['dropped'].sum()) == 0 and (buf['ids'] >= 0).all()      # the front face fills the screen


# ---- shading -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('names,views,size', [
    (('sphere',), (0, 12, _key(FREE_POSE)), 64),
    (('cube', 'soup'), (5, 17), 37),
    (('torus',), (_key(CLOSE_POSE),), 64),
])
def test_shading_within_one_level_of_float64(names, views, size):
    img, buf = run(names, views, size)
    ps = poses([v if isinstance(v, int) else np.array(v).reshape(4, 4) for v in views])
    for b, name in enumerate(names):
        v, f = mesh(name)
        for j in range(len(views)):
            want = O.shade(v, f, buf['ids'][b, j], ps[j], size, buf['norm'][b, :3], buf['norm'][b, 3])
            assert np.abs(img[b, j].astype(int) - want.astype(int)).max() <= 1
            bg = buf['ids'][b, j] < 0
            assert bg.any() or name == 'torus'
            assert (img[b, j][bg] == 255).all()
            lit = img[b, j][~bg]
            assert lit.size and lit.max() > 40 and (lit[:, 0] == lit[:, 1]).all()      # grey material: r = g = b


def test_background_and_material_are_parameters():
    from octfusion_amd import render as R
    v, f = mesh('cube')
    ps = poses([1])
    img, buf = R.render([(v, f)], poses=ps, size=37, buffers=True, background=(0.0, 0.5, 1.0), roughness=0.4,
                        base_color=(0.8, 0.3, 0.1), metallic=0.6, spot=0.0)
    ids = buf['ids'][0, 0].cpu().numpy()
    want = O.shade(v, f, ids, ps[0], 37, buf['norm'][0, :3].cpu().numpy(), float(buf['norm'][0, 3]),
                   background=(0.0, 0.5, 1.0), roughness=0.4, base_color=(0.8, 0.3, 0.1), metallic=0.6, spot=0.0)
    got = img[0, 0].cpu().numpy()
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert (got[ids < 0] == np.array([0, 128, 255], np.uint8)).all()
    lit = got[ids >= 0].astype(int)
    assert (lit[:, 0] >= lit[:, 2]).all() and (lit[:, 0] > lit[:, 2]).any()
    with pytest.raises(TypeError):
        R.render([(v, f)], poses=ps, size=8, shininess=3)


def test_reversed_winding_gives_the_same_image():
    from octfusion_amd import render as R
    for name in ('sphere', 'soup'):
        v, f = mesh(name)
        a, ba = R.render([(v, f)], poses=poses([3, 14]), size=64, buffers=True)
        b, bb = R.render([(v, np.ascontiguousarray(f[:, ::-1]))], poses=poses([3, 14]), size=64, buffers=True)
        assert torch.equal(ba['ids'], bb['ids']) and torch.equal(ba['depth'], bb['depth'])
        assert torch.equal(a, b)


# ---- invariance ----------------------------------------------------------------------------------------------------
def test_runs_batches_and_view_subsets_are_bit_equal():
    from octfusion_amd import render as R
    size = 64
    meshes = [mesh('cube'), mesh('torus'), mesh('sphere')]
    full, fb = R.render(meshes, size=size, buffers=True)                      # the 20 views
    again, ab = R.render(meshes, size=size, buffers=True)
    assert full.shape == (3, 20, size, size, 3) and full.dtype == torch.uint8
    assert torch.equal(full, again) and all(torch.equal(fb[k], ab[k]) for k in fb)
    alone, sb = R.render([meshes[1]], size=size, buffers=True)                # the middle of the batch, alone
    assert torch.equal(alone[0], full[1]) and torch.equal(sb['ids'][0], fb['ids'][1])
    assert torch.equal(sb['depth'][0], fb['depth'][1])
    one, ob = R.render(meshes, poses=poses([13]), size=size, buffers=True)    # one view, alone
    assert torch.equal(one[:, 0], full[:, 13]) and torch.equal(ob['ids'][:, 0], fb['ids'][:, 13])
    # chunking over views does not show
    saved = R.WORKSPACE_BYTES
    try:
        R.WORKSPACE_BYTES = 7 * (3 * size * size * 8 + fb['sxy'].shape[1] * 16 + sum(len(m[1]) for m in meshes) * 8)
        chunked, cb = R.render(meshes, size=size, buffers=True)
    finally:
        R.WORKSPACE_BYTES = saved
    assert torch.equal(chunked, full) and all(torch.equal(fb[k], cb[k]) for k in fb)


# ---- analytic ------------------------------------------------------------------------------------------------------
def test_unit_sphere_covers_the_analytic_disc():
    """After normalisation the mesh lies inside the unit ball about the origin and, being closed around it, contains
    the ball of radius rho = the least distance from the origin to a face's plane.  A ball of radius s about the
    look-at target at eye distance d projects to the disc of radius (size / 2) tan(asin(s / d)) / tan 30 about the
    image centre, so the silhouette lies between the discs of radius R(rho) and R(1).  The number of pixel centres in
    a disc of radius R is within pi (sqrt2 R + 1/2) < 2 pi R of its area (every such pixel square lies within sqrt2 / 2
    of the disc's boundary or inside it).  Hence |covered - pi R(1)^2| <= pi (R(1)^2 - R(rho)^2) + 2 pi R(1): the
    tessellation's chord error plus one pixel along the circumference (snapping moves an edge by < 1/256 pixel)."""
    size = 96
    name = 'sphere32'
    _, buf = run((name,), (0,), size)
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
    covered = buf['ids'][0, 0] >= 0
    bound = math.pi * (R1 * R1 - Rr * Rr) + 2 * math.pi * R1
    assert abs(int(covered.sum()) - math.pi * R1 * R1) <= bound
    ys, xs = np.nonzero(covered)
    assert abs(xs.mean() + 0.5 - size / 2) < 0.5 and abs(ys.mean() + 0.5 - size / 2) < 0.5
    rr = np.hypot(xs + 0.5 - size / 2, ys + 0.5 - size / 2)
    assert rr.max() <= R1 + 1 / 256 + 1e-9                  # nothing outside the unit ball's disc


# ---- validation ----------------------------------------------------------------------------------------------------
def test_bad_meshes_raise_before_any_launch():
    from octfusion_amd import render as R
    v, f = mesh('cube')
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(ValueError, match=r'shape 1 .*face index outside \[0, 8\)'):
        R.render([(v, f), (v, bad)], size=16)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match='shape 0'):
        R.render([(v, bad)], size=16)
    with pytest.raises(ValueError, match='shape 1 has no faces'):
        R.render([(v, f), (v, np.zeros((0, 3), np.int32))], size=16)
    with pytest.raises(ValueError):
        R.render([], size=16)
    with pytest.raises(ValueError):
        R.render([(v, f)], size=0)
    # non-finite vertices: their triangles are dropped and counted, the rest renders
    w = v.copy()
    w[7] = np.nan
    img, buf = R.render([(w, f)], poses=poses([0]), size=37, buffers=True)
    assert int(buf['dropped'][0, 0]) == int((f == 7).any(1).sum())
    keys, dropped = O.raster(buf['sxy'][0].cpu().numpy(), buf['vertex_depth'][0].cpu().numpy(), f, 37)
    assert np.array_equal(buf['ids'][0, 0].cpu().numpy(), O.split_keys(keys)[0])


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_cli_writes_the_reference_layout(tmp_path, capsys):
    from octfusion_amd import mesh as PM, render as R
    src = tmp_path / 'objs'
    for name in ('cube', 'sphere'):
        PM.write_obj(str(src / (name + '.obj')), *mesh(name))
    out = tmp_path / 'fid'
    res = R.main(['--input', str(src), '--out', str(out), '--size', '37', '--batch', '2'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
    rec = json.loads(line)
    assert rec['shapes'] == 2 and rec['dropped_triangles'] == 0 and rec['seconds'] > 0 and res['shapes'] == 2
    want = R.render([PM.read_obj(str(src / 'cube.obj')), PM.read_obj(str(src / 'sphere.obj'))], size=37).cpu().numpy()
    assert sorted(os.listdir(out)) == sorted('view_%d' % j for j in range(20))
    for j in range(20):
        assert sorted(os.listdir(out / ('view_%d' % j))) == ['cube.png', 'sphere.png']
        for b, name in enumerate(('cube', 'sphere')):
            got = _inflate_png(open(out / ('view_%d' % j) / (name + '.png'), 'rb').read())
            assert np.array_equal(got, want[b, j])
    # a file list and a batch of one give the same files
    out2 = tmp_path / 'fid2'
    R.main(['--input', str(src / 'sphere.obj'), str(src / 'cube.obj'), '--out', str(out2), '--size', '37', '--batch', '1'])
    for name in ('cube', 'sphere'):
        assert open(out2 / 'view_11' / (name + '.png'), 'rb').read() == open(out / 'view_11' / (name + '.png'), 'rb').read()


def test_generate_cli_writes_fid_images(tmp_path, capsys):
    from octfusion_amd import configs, generate as G, mesh as PM, render as R
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    PM.MESH_SCALES['tiny_uncond'] = PM.MESH_SCALES['snet_uncond']
    out_dir = str(tmp_path / 'gen')
    res = G.main(['--config', 'tiny_uncond', '--shapes', '3', '--steps', '4', '--batch', '2', '--sdf-resolution', '64',
                  '--seed', '5', '--mesh', '--views', '--out', out_dir])
    written = 0
    for i in res['rank0_indices']:
        obj = os.path.join(out_dir, '%d.obj' % i)
        pngs = [os.path.join(out_dir, 'fid_images', 'view_%d' % j, '%d.png' % i) for j in range(20)]
        assert all(os.path.exists(p) == os.path.exists(obj) for p in pngs)
        if not os.path.exists(obj):
            continue
        # the OBJ round trip is exact, so rendering the written mesh gives the written images
        want = R.render([PM.read_obj(obj)]).cpu().numpy()
        assert want.shape == (1, 20, 299, 299, 3)
        for j in (0, 13):
            assert np.array_equal(_inflate_png(open(pngs[j], 'rb').read()), want[0, j])
        written += 1
    assert written > 0
    with pytest.raises(ValueError):
        G.main(['--config', 'tiny_uncond', '--shapes', '1', '--views'])
