"""GPU tests of the mesh -> SDF lattice (csrc/ofx_mesh2sdf.hip, octfusion_amd/mesh2sdf.py) against the float64 oracle
(tests/mesh2sdf_oracle.py: brute-force closest point, winding-number sign).

Tolerances.
  values  |got - oracle| <= 1e-5 + 1e-5 |oracle|.  Coordinates are <= 2 in magnitude, an fp32 ulp is 2^-23, and a
          closest-point evaluation is a few tens of operations: a few 1e-6 absolute even in fp32, also near zero
          distance where the error of the projected point dominates.  (The kernel evaluates in fp64 and rounds once,
          so what is left is the fp32 rounding of the result, <= 2^-24 |value|, and the lattice coordinate.)
  signs   equal to the oracle's at every lattice point whose oracle distance is >= 1e-5; at most 0.1 % of the points
          may be left out (the rule of test_gpu_sdfdata.py).
  driver  dataset.prepare_shape's samples against the oracle's distance to the SAVED mesh at the sample positions:
          |sdf_sample - oracle| <= fp16 ulp + interpolation + position.
            fp16 ulp      the stored value is rounded to fp16: |v| < 2 here, so one ulp is at most 2^-10 = 9.8e-4
                          (a full ulp, not half: the rule of test_gpu_sdfdata.py);
            interpolation a signed distance field is 1-Lipschitz: inside a cell of edge h = 2 / S the trilinear value
                          is a convex combination of corner values, each within the cell diagonal sqrt(3) h of the
                          value at the sample, and so is the interpolant: <= sqrt(3) * 2 / 32 = 0.1083 at S = 32;
            position      the sample position is itself stored in fp16 (half an ulp of 2^-11 per axis on the lattice's
                          scale, sqrt(3) * 2^-12 together): <= 2^-10 by the Lipschitz property;
            lattice       the lattice values themselves: 1e-5 (above).
          The bound used is their sum, 0.1102.  It is coarse because S = 32 is coarse, not because the check is loose:
          the same derivation gives 0.029 at the real S = 128.  The driver runs with --level 0.1 (1.6 cells, as the
          repair test): the default 0.015 is one cell at S = 128 and a quarter of a cell here.
"""
import os

import numpy as np
import pytest
import torch

import mesh2sdf_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

C = (0.07, -0.05, 0.03)
R = 0.55
TC = (0.03, 0.02, -0.04)


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.asarray(v, np.float32)).to(dev()), torch.from_numpy(np.asarray(f, np.int32)).to(dev()))


def run(meshes, S, signed=True):
    from octfusion_amd import mesh2sdf as M
    out = M.mesh_to_sdf([to_dev(m) for m in meshes], S, signed)
    assert out.shape == (len(meshes), S, S, S) and out.dtype == torch.float32
    return out


def flat(t):
    return t.cpu().numpy().astype(np.float64).reshape(-1)


def check_values(got, ref, what):
    err = np.abs(got - ref)
    worst = (err - 1e-5 * np.abs(ref)).max()
    print('%s: max |got - oracle| = %.3e over %d points' % (what, err.max(), len(ref)))
    assert np.isfinite(got).all()
    assert worst <= 1e-5


def check_signs(got, inside, d, what, max_out=0.001):
    ok = d >= 1e-5
    left_out = int((~ok).sum())
    wrong = int(((got < 0) != inside)[ok].sum())
    print('%s: %d of %d points left out of the sign check, %d wrong' % (what, left_out, len(d), wrong))
    assert left_out <= max_out * len(d)
    assert wrong == 0
    return left_out


def check_mesh(m, S, what):
    """Signed and unsigned lattices of one mesh against the oracle on the whole lattice."""
    P = O.lattice(S)
    d = O.udf(P, *m)
    inside = O.inside(P, *m)
    u = flat(run([m], S, signed=False))
    s = flat(run([m], S, signed=True))
    assert (u >= 0).all()
    check_values(u, d, what + ' unsigned')
    check_values(np.abs(s), d, what + ' signed')
    assert np.array_equal(np.abs(s), u)
    return check_signs(s, inside, d, what), s, d


@pytest.fixture(scope='module')
def sphere():
    m = O.icosphere(2, C, R)
    P = O.lattice(16)
    return {'mesh': m, 'udf': O.udf(P, *m), 'inside': O.inside(P, *m)}


@pytest.fixture(scope='module')
def torus():
    m = O.torus(16, 8, 0.5, 0.2, TC)
    P = O.lattice(16)
    return {'mesh': m, 'udf': O.udf(P, *m), 'inside': O.inside(P, *m)}


# ---- 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['sphere', 'torus'])
def test_sphere_and_torus(which, sphere, torus):
    c = {'sphere': sphere, 'torus': torus}[which]
    assert len(c['mesh'][1]) == {'sphere': 320, 'torus': 256}[which]
    u = flat(run([c['mesh']], 16, signed=False))
    s = flat(run([c['mesh']], 16, signed=True))
    check_values(u, c['udf'], which + ' unsigned')
    check_values(np.abs(s), c['udf'], which + ' signed')
    left = check_signs(s, c['inside'], c['udf'], which)
    assert left <= 1


# ---- 2 ------------------------------------------------------------------------------------------------------------
def test_lattice_aligned_box():
    m = O.box(-0.5, 0.5)
    P = O.lattice(16)
    d = O.udf(P, *m)
    s = flat(run([m], 16))
    check_values(np.abs(s), d, 'aligned box')
    surface = d < 1e-5
    assert int(surface.sum()) == 386
    i = np.rint((P + 1) * 8).astype(int)
    interior = ((i > 4) & (i < 12)).all(1)
    assert int(interior.sum()) == 343
    assert (s[interior] < 0).all()
    rest = ~surface & ~interior
    print('aligned box: %d points outside, %d of them negative' % (rest.sum(), (s[rest] < 0).sum()))
    assert (s[rest] > 0).all()


# ---- 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [16, 20])
def test_big_triangles_and_odd_sizes(S):
    """Triangles that span every brick and bin, and a lattice size that is no multiple of a brick (4), a column tile
    (8) or a bin (8 cells).  At S = 20 the planes +-0.9 are lattice planes (2 * 19 / 20 - 1), where a quarter of the
    lattice sits on the surface and has no sign: there the 0.9 box is checked for its values, and the same box at
    +-0.85, between two lattice planes, for values and signs."""
    if S == 16:
        check_mesh(O.box(-0.9, 0.9), S, 'box 0.9, S = 16')
    else:
        m = O.box(-0.9, 0.9)
        check_values(flat(run([m], S, signed=False)), O.udf(O.lattice(S), *m), 'box 0.9, S = 20 unsigned')
        check_mesh(O.box(-0.85, 0.85), S, 'box 0.85, S = 20')
    # the sphere leaves the lattice through the -x wall: crossings at x < -1 still flip their columns
    m = O.icosphere(2, (-0.7, 0.1, 0.0), 0.5)
    assert m[0][:, 0].min() < -1.0
    _, s, d = check_mesh(m, S, 'shifted sphere, S = %d' % S)
    assert (s.reshape(S, S, S)[0] < 0).sum() > 0              # inside already at the wall


# ---- 4 ------------------------------------------------------------------------------------------------------------
def test_nested_boxes():
    m = O.merge(O.box(-0.6, 0.6), O.box(-0.3, 0.3))
    _, s, d = check_mesh(m, 16, 'nested boxes')
    P = O.lattice(16)
    cavity = (np.abs(P) < 0.3).all(1)
    wall = (np.abs(P) < 0.6).all(1) & ~cavity
    assert (s[cavity] > 0).all() and (s[wall] < 0).all()


# ---- 5 ------------------------------------------------------------------------------------------------------------
def test_many_triangles():
    S = 32
    V, F = O.icosphere(4, C, R)
    assert len(F) == 5120
    s = flat(run([(V, F)], S))
    P = O.lattice(S)
    pick = np.random.RandomState(5).choice(S ** 3, 512, replace=False)
    check_values(np.abs(s[pick]), O.udf(P[pick], V, F), 'icosphere(4) on 512 points')
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cc = np.asarray(C)
    r_in = np.abs(((a - cc) * n).sum(1)).min()
    q = np.linalg.norm(P - cc, axis=1)
    clear = np.abs(q - R) > (R - r_in) + 1e-6                 # the mesh lies between the spheres r_in and R
    print('icosphere(4): R - r_in = %.2e, %d of %d points checked for sign' % (R - r_in, clear.sum(), len(q)))
    assert clear.sum() > 0.95 * len(q)
    assert np.array_equal(s[clear] < 0, q[clear] < R)


# ---- 6 ------------------------------------------------------------------------------------------------------------
def test_degenerate_triangles(sphere):
    V, F = sphere['mesh']
    # near the sphere's centre, on exactly representable coordinates: a repeated vertex, a collinear triple, a point
    extra = np.array([[0.0625, -0.0625, 0.03125], [0.125, -0.0625, 0.0625], [0.1875, -0.0625, 0.09375],
                      [0.0625, 0.03125, 0.03125]])
    assert (np.cross(extra[1] - extra[0], extra[2] - extra[0]) == 0).all()
    Fe = np.asarray([[0, 0, 3], [0, 1, 2], [3, 3, 3]], np.int32)
    n = len(V)
    V2, F2 = np.concatenate([V, extra]), np.concatenate([F, Fe + n])
    P = O.lattice(16)
    de = O.udf(P, extra, Fe)
    d2 = np.minimum(de, sphere['udf'])
    u1 = run([(V, F)], 16, signed=False)
    u2 = run([(V2, F2)], 16, signed=False)
    s2 = run([(V2, F2)], 16, signed=True)
    assert torch.isfinite(u2).all() and torch.isfinite(s2).all()
    check_values(flat(u2), d2, 'sphere + zero-area triangles')
    check_values(flat(run([(extra, Fe)], 16, signed=False)), de, 'zero-area triangles alone')
    nearer = de < sphere['udf']
    print('zero-area triangles are the nearest at %d points' % nearer.sum())
    assert 10 < nearer.sum() < 400                            # the extras win only around the centre
    same = torch.from_numpy(de > sphere['udf'] + 1e-6).to(dev()).view(16, 16, 16)
    assert torch.equal(u1[0][same].view(torch.int32), u2[0][same].view(torch.int32))
    # zero-area triangles never count as crossings
    s1 = run([(V, F)], 16, signed=True)
    assert torch.equal(s1 < 0, s2 < 0)


def test_bad_input(sphere, torus):
    from octfusion_amd import mesh2sdf as M
    V, F = sphere['mesh']
    good = to_dev(torus['mesh'])
    Fb = F.copy()
    Fb[17, 1] = len(V)                                        # one past the end
    with pytest.raises(ValueError, match='shape 1'):
        M.mesh_to_sdf([good, to_dev((V, Fb))], 16)
    Fb[17, 1] = -1
    with pytest.raises(ValueError, match='shape 0'):
        M.mesh_to_sdf([to_dev((V, Fb)), good], 16)
    Vn = V.copy()
    Vn[int(F[5, 2]), 1] = np.nan
    with pytest.raises(ValueError, match='shape 1'):
        M.mesh_to_sdf([good, to_dev((Vn, F))], 16)
    Vu = np.concatenate([V, [[np.nan, 0.0, 0.0]]])            # a bad vertex no face uses is nobody's business
    assert torch.equal(M.mesh_to_sdf([to_dev((Vu, F))], 16), M.mesh_to_sdf([to_dev((V, F))], 16))
    empty = (good[0], good[1][:0])
    with pytest.raises(ValueError, match='shape 1 has no faces'):
        M.mesh_to_sdf([good, empty], 16)
    with pytest.raises(ValueError):
        M.mesh_to_sdf([good], 1)
    torch.cuda.synchronize()


# ---- 7 ------------------------------------------------------------------------------------------------------------
def test_batch_and_determinism(sphere, torus):
    meshes = [torus['mesh'], O.box(-0.5, 0.5), sphere['mesh']]
    assert len({len(m[0]) for m in meshes}) == 3 and len({len(m[1]) for m in meshes}) == 3
    for signed in (True, False):
        both = run(meshes, 16, signed)
        again = run(meshes, 16, signed)
        assert torch.equal(both.view(torch.int32), again.view(torch.int32))
        for k, m in enumerate(meshes):
            alone = run([m], 16, signed)
            assert torch.equal(alone[0].view(torch.int32), both[k].view(torch.int32)), 'shape %d' % k
    check_values(np.abs(flat(both[0])), torus['udf'], 'torus in a batch')
    check_values(np.abs(flat(both[2])), sphere['udf'], 'sphere in a batch')


# ---- 8 ------------------------------------------------------------------------------------------------------------
def test_open_mesh():
    m = O.plate()
    P = O.lattice(16)
    check_values(flat(run([m], 16, signed=False)), O.udf(P, *m), 'plate')


# ---- 9 ------------------------------------------------------------------------------------------------------------
def edge_face_counts(faces):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


@pytest.mark.parametrize('which', ['plate', 'sphere'])
def test_repair(which):
    from octfusion_amd import mesh as ME, mesh2sdf as M
    S, level = 32, 0.1
    m = O.plate() if which == 'plate' else O.icosphere(2, (0.0, 0.0, 0.0), 0.5)
    dm = to_dev(m)
    sdf, (mv, mf) = M.compute(dm[0], dm[1], S, fix=True, level=level, return_mesh=True)
    assert sdf.shape == (S, S, S) and sdf.dtype == torch.float32
    # the composition of the public calls, step by step
    u = M.mesh_to_sdf([dm], S, signed=False)
    shell = ME.largest_component(ME.marching_cubes(u, level, bbmin=-1, bbmax=1))[0]
    assert torch.equal(shell[0].view(torch.int32), mv.view(torch.int32)) and torch.equal(shell[1], mf)
    assert torch.equal(M.mesh_to_sdf([shell], S, signed=True)[0].view(torch.int32), sdf.view(torch.int32))
    # numpy in, and the lattice alone
    assert torch.equal(M.compute(m[0], m[1], S, True, level).view(torch.int32), sdf.view(torch.int32))
    # watertight: every edge has exactly two faces
    cnt = edge_face_counts(mf.cpu().numpy())
    print('%s: repaired mesh %d vertices, %d faces' % (which, mv.shape[0], mf.shape[0]))
    assert (cnt == 2).all()
    P = O.lattice(S)
    s = flat(sdf)
    if which == 'sphere':                                     # 32^3 x 320 pairs is too slow for a test: a fixed quarter
        sub = np.sort(np.random.RandomState(90).choice(S ** 3, 8192, replace=False))
        P, s = P[sub], s[sub]
    d = O.udf(P, *m)
    assert (d < level - 1e-5).sum() > 100
    assert (s[d < level - 1e-5] < 0).all()
    band = np.abs(d - level) < 1e-5
    assert band.sum() <= 0.001 * len(d)
    if which == 'plate':
        assert (s[d > level + 1e-5] > 0).all()
    else:
        solid = (d < level) | (np.linalg.norm(P, axis=1) < 0.5)
        assert np.array_equal(s[~band] < 0, solid[~band])
    pick = np.random.RandomState(9).choice(len(P), 512, replace=False)
    ref = O.udf(P[pick], mv.cpu().numpy().astype(np.float64), mf.cpu().numpy())
    check_values(np.abs(s[pick]), ref, which + ' repaired, 512 points')


# ---- 10 -----------------------------------------------------------------------------------------------------------
def test_driver(tmp_path):
    from octfusion_amd import dataset as D, mesh2sdf as M
    V, F = O.icosphere(2, (0.3, -0.2, 0.5), 1.7)              # raw coordinates: normalize has work to do
    src = tmp_path / 'raw' / 'ball.obj'
    src.parent.mkdir()
    nV = len(V)
    # faces 0 and 1 of an icosphere(2) share an edge?  Build the quad from face 0 and the face across its edge (b, c).
    a, b, c = (int(i) for i in F[0])
    other = [k for k in range(1, len(F)) if {b, c} <= set(int(i) for i in F[k])]
    assert len(other) == 1
    d = [int(i) for i in F[other[0]] if int(i) not in (b, c)][0]
    rest = [k for k in range(1, len(F)) if k != other[0]]
    with open(src, 'w') as fh:
        fh.write('# test mesh\nmtllib none.mtl\n')
        for p in V:
            fh.write('v %.9g %.9g %.9g\n' % tuple(p))
        fh.write('vt 0.5 0.5\nvn 0 0 1\ng ball\n')
        fh.write('f %d/1/1 %d/1/1 %d/1/1 %d/1/1\n' % (a + 1, b + 1, d + 1, c + 1))          # the quad a b d c
        k0 = rest[0]
        fh.write('f %d//1 %d//1 %d//1\n' % (int(F[k0, 0]) - nV, int(F[k0, 1]) + 1, int(F[k0, 2]) + 1))   # negative
        for k in rest[1:]:
            fh.write('f %d/1 %d/1 %d/1\n' % tuple(int(i) + 1 for i in F[k]))
    rv, rf = M.read_mesh(str(src))
    assert rv.shape == (nV, 3) and rf.shape == (len(F), 3) and rf.dtype == np.int32 and rv.dtype == np.float32
    assert np.array_equal(rv, V.astype(np.float32))
    assert sorted(map(tuple, np.sort(rf[2:], axis=1))) == sorted(map(tuple, np.sort(F[rest], axis=1)))
    assert np.abs(O.winding(np.asarray([[0.3, -0.2, 0.5]]), rv.astype(np.float64), rf)).round() == 1   # still closed

    root = tmp_path / 'out'
    S = 32
    M.main(['--input', str(src), '--out', str(root), '--size', str(S), '--level', '0.1', '--pointcloud',
            '--points', '4096'])
    f_sdf, f_obj, f_box = root / 'sdf' / 'ball.npy', root / 'mesh' / 'ball.obj', root / 'bbox' / 'ball.npz'
    f_pc = root / 'dataset' / 'ball' / 'pointcloud.npz'
    for p in (f_sdf, f_obj, f_box, f_pc):
        assert p.exists(), p
    lat = np.load(f_sdf)
    assert lat.shape == (S, S, S) and lat.dtype == np.float32 and np.isfinite(lat).all()
    with np.load(f_box) as z:
        assert sorted(z.files) == ['bbmax', 'bbmin', 'mul']
        bbmin, bbmax, mul = z['bbmin'], z['bbmax'], float(z['mul'])
    vn, nmin, nmax = M.normalize(rv)
    assert mul == 0.8 and np.array_equal(bbmin, nmin) and np.array_equal(bbmax, nmax)
    assert np.array_equal(bbmin, rv.astype(np.float64).min(0)) and np.array_equal(bbmax, rv.astype(np.float64).max(0))
    assert np.isclose(np.abs(vn).max(), 0.8, rtol=0, atol=1e-12) and np.allclose(vn.min(0) + vn.max(0), 0, atol=1e-12)
    with np.load(f_pc) as z:
        assert sorted(z.files) == ['normals', 'points']
        pts, nrm = z['points'], z['normals']
    assert pts.shape == (4096, 3) and nrm.shape == (4096, 3) and pts.dtype == np.float16 and nrm.dtype == np.float16
    from octfusion_amd import mesh as ME
    mv, mf = ME.read_obj(str(f_obj))
    assert (edge_face_counts(mf) == 2).all()
    assert np.abs(mv).max() <= 0.5                            # vertices * shape_scale
    mv2 = mv.astype(np.float64) / 0.5                         # back on the lattice's scale
    some = np.random.RandomState(10).choice(len(pts), 512, replace=False)       # the oracle is brute force
    dp = O.udf(pts[some].astype(np.float64) / 0.5, mv2, mf)
    print('driver: cloud at most %.2e off the saved mesh' % dp.max())
    assert dp.max() <= 2.0 ** -10 * 2                         # fp16 positions, three axes
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 2e-3

    # the files are what the next step reads
    written = D.prepare_shape(str(f_sdf), str(f_pc.parent), 'ball', depth=5, full_depth=3)
    assert [os.path.basename(w) for w in written] == ['sdf.npz']
    sample = D.ReadFile({'load_sdf': True, 'load_pointcloud': True})(str(f_pc.parent))
    sp = sample['sdf']['points'].astype(np.float64) / 0.5
    sv = sample['sdf']['sdf'].astype(np.float64)
    assert len(sv) > 1000
    some = np.random.RandomState(11).choice(len(sv), 512, replace=False)
    sp, sv = sp[some], sv[some]
    ref, _ = O.sdf(sp, mv2, mf)
    bound = 2.0 ** -10 + np.sqrt(3.0) * 2 / S + 2.0 ** -10 + 1e-5
    err = np.abs(sv - ref)
    print('driver: %d samples, max |sdf - oracle| = %.3e (bound %.4f), mean %.3e' % (len(sv), err.max(), bound, err.mean()))
    assert err.max() <= bound
