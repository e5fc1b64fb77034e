"""GPU checks of the reconstruction scores (octfusion_amd.recon_metrics.surface_scores / occupancy_iou) and of the
driver's --metrics / --occupancy records, against the float64 oracle tests/recon_metrics_oracle.py.

Tolerances.  On lattice-valued clouds (coordinates k / 64) every fp32 distance is exact, so the device and the float64
oracle reduce the same numbers: the threshold counts must be equal, and the float64 means differ only by the order of
their sums -- n * 2^-53 relative at worst on non-negative terms, 3e-13 for n = 3000, inside the 1e-12 asked.
Concentric spheres: the sampling spacing sqrt(area / n) bounds how far the mean nearest-sample distance can lie from
the gap delta (the marching-cubes surface itself is within step^2 / (8 r), far below it)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import common as C
import mc_oracle as MC
import recon_metrics_oracle as MO
import recon_oracle as RO
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KEYS = ['completeness', 'accuracy', 'completeness2', 'accuracy2', 'chamfer_l1', 'chamfer_l2', 'normals_completeness',
        'normals_accuracy', 'normal_consistency']


def _unit(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _lattice_pair():
    rng = np.random.default_rng(3)
    gt = rng.integers(-128, 129, (3000, 3))
    moved = gt[rng.permutation(3000)[:2200]] + rng.integers(-4, 5, (2200, 3))
    pred = np.concatenate([moved, rng.integers(-128, 129, (300, 3)), gt[:77]])
    f = np.float32(64)
    return (gt.astype(np.float32) / f, _unit(3000, 4)), (pred.astype(np.float32) / f, _unit(len(pred), 5))


def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_lattice_clouds_match_the_oracle():
    from octfusion_amd import recon_metrics as RM
    gt, pred = _lattice_pair()
    taus = (0.03, 0.05, 0.1, 1e-4)                    # tau^2 * 4096 = 3.6864, 10.24, 40.96, 4.1e-5: no integer
    for t in taus:
        assert abs(t * t * 4096 - round(t * t * 4096)) > 1e-6
    want = MO.surface_scores(gt, pred, taus)
    tg, tp = [tuple(torch.from_numpy(x).to(dev()) for x in s) for s in (gt, pred)]
    got = RM.surface_scores(tg, tp, thresholds=taus)
    assert set(got) == set(want) and got['thresholds'] == list(taus)
    for k in KEYS:
        assert _close(got[k], want[k]), (k, got[k], want[k])
    for k, n in (('recall', len(gt[0])), ('precision', len(pred[0]))):
        for a, b in zip(got[k], want[k]):
            assert round(a * n) == round(b * n) and _close(a, b), (k, a, b)
    for a, b in zip(got['fscore'], want['fscore']):
        assert _close(a, b)
    assert 0 < want['recall'][0] < want['recall'][1] < want['recall'][2] < 1 and want['recall'][3] > 0.02
    # a list of pairs scores each pair as the single call does
    both = RM.surface_scores([tg, tp], [tp, tg], thresholds=taus)
    assert both[0] == got and both[1]['recall'] == got['precision'] and both[1]['accuracy'] == got['completeness']


def test_a_mesh_against_itself():
    from octfusion_amd import recon_metrics as RM
    m = tuple(torch.from_numpy(x).to(dev()) for x in RO.cube_mesh(0.4, (0.1, -0.05, 0.02)))
    s = RM.surface_scores(m, m, n=5000, seed=3)
    assert s['chamfer_l1'] == 0.0 and s['chamfer_l2'] == 0.0 and s['completeness'] == 0.0 and s['accuracy'] == 0.0
    assert s['fscore'] == [1.0, 1.0, 1.0] and s['recall'] == [1.0] * 3 and s['precision'] == [1.0] * 3
    assert s['normal_consistency'] == 1.0             # the cube's normals are exact unit vectors


def test_concentric_spheres():
    from octfusion_amd import mesh, recon_metrics as RM
    R, r, delta, n = 64, 0.5, 0.1, 20000
    sdf = torch.from_numpy(np.stack([MC.sphere(R, r), MC.sphere(R, r + delta)])).to(dev())
    inner, outer = mesh.marching_cubes(sdf)
    spacing = math.sqrt(4 * math.pi * (r + delta) ** 2 / n)
    assert spacing < delta / 4
    s = RM.surface_scores(inner, outer, n=n, seed=1, thresholds=(delta / 2, 2 * delta))
    print('completeness %.5f accuracy %.5f (delta %.3f, spacing %.4f)' % (s['completeness'], s['accuracy'], delta, spacing))
    assert abs(s['completeness'] - delta) <= spacing and abs(s['accuracy'] - delta) <= spacing
    assert s['fscore'] == [0.0, 1.0]
    assert s['normal_consistency'] > 0.99             # radial normals, nearest point along the radius


def _sphere_field(radius, centre=(0.05, -0.1, 0.02)):
    c = torch.tensor(centre, dtype=torch.float32, device=dev())

    def field(pos):
        assert pos.shape[1] == 4 and pos.dtype == torch.float32 and bool((pos[:, 3] == 2).all())
        return (pos[:, :3] - c).norm(dim=1) - radius
    return field


def test_occupancy_iou_against_sampled_occupancies():
    from octfusion_amd import dataset, recon_metrics as RM
    ps, n = 0.5, 1003                                  # n is not a multiple of 8
    occ = dataset.sample_occu(MC.sphere(32, 0.6), n=n, seed=5, shape_id=9, shape_scale=ps)
    field = _sphere_field(0.45)
    got = RM.occupancy_iou(field, occ['points'], occ['occupancies'], ps, batch_index=2)
    pos = torch.cat([occ['points'].float() / ps, torch.full((n, 1), 2.0, device=dev())], 1)
    values = field(pos).cpu().numpy()
    bits = occ['occupancies'].cpu().numpy()
    want = MO.occupancy_iou(values, bits)
    assert got == want and 0 < want[1] < want[2] < n
    # numpy inputs (what the driver reads from points.npz) and another level
    got = RM.occupancy_iou(field, occ['points'].cpu().numpy(), bits, ps, level=0.1, batch_index=2)
    assert got == MO.occupancy_iou(values, bits, level=0.1) and got[1] > want[1]
    # nothing occupied on either side
    assert RM.occupancy_iou(_sphere_field(-1.0), occ['points'], torch.zeros_like(occ['occupancies']), ps,
                            batch_index=2) == (None, 0, 0)
    with pytest.raises(ValueError):
        RM.occupancy_iou(field, occ['points'], occ['occupancies'][:-1], ps, batch_index=2)


def test_driver_records(golden, tmp_path):
    """The tiny VAE of test_gpu_reconstruct.py on two point-cloud inputs in one batch, the second with a points.npz."""
    from octfusion_amd import dataset, reconstruct as R, recon_metrics as RM, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    from test_gpu_reconstruct import _box_points
    kw = {k: v for k, v in golden('g_vae_enc')['cfg'].items()}
    ps, npts = 0.5, 2048
    sp, sn = C.surface_points(4000, 9, 'sphere')
    bp, bn = _box_points(4000, 0.6, 3)
    clouds = {}
    for name, p, n in (('ball', sp.numpy(), sn.numpy()), ('box', bp, bn)):
        d = tmp_path / 'data' / name
        d.mkdir(parents=True)
        np.savez(str(d / 'pointcloud.npz'), points=p * ps, normals=n)
        q = torch.from_numpy(p * np.float32(ps)).to(dev()) / ps
        keep = ((q > -1) & (q < 1)).all(1)
        clouds[name] = (q[keep], torch.from_numpy(n).to(dev())[keep])
    occ = dataset.sample_occu(MC.sphere(32, 0.55), n=1003, seed=1, shape_id=2, shape_scale=ps)
    dataset.write_occu_npz(str(tmp_path / 'data' / 'box' / 'points.npz'), occ)
    vae = GraphVAE(**kw)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cfg = {'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': ps}
    inputs = R.read_inputs([str(tmp_path / 'data' / 'ball'), str(tmp_path / 'data' / 'box')])
    args = dict(sdf_resolution=32, batch=2, seed=4, chamfer_points=npts)
    plain = R.reconstruct(vae, cfg, inputs, dev(), out_dir=str(tmp_path / 'plain'), **args)
    today = {'gt', 'input_points', 'vertices', 'faces', 'chamfer_a', 'chamfer_b', 'obj'}
    saved = json.load(open(os.path.join(str(tmp_path / 'plain'), 'metrics.json')))
    assert all(set(rec) == today for rec in saved['shapes'].values()) and 'fields' not in plain
    assert set(saved) == {'config', 'point_scale', 'sdf_resolution', 'sdf_scale', 'mpu_depth', 'fit', 'seed',
                          'chamfer_points', 'chamfer_scale', 'shapes'}
    taus = (0.02, 0.05)
    with pytest.warns(UserWarning, match='ball: no points.npz'):
        res = R.reconstruct(vae, cfg, inputs, dev(), out_dir=str(tmp_path / 'full'), metrics=True, thresholds=taus,
                            occupancy=True, **args)
    saved = json.load(open(os.path.join(str(tmp_path / 'full'), 'metrics.json')))
    new = {'scores', 'iou', 'iou_intersection', 'iou_union'}
    for k, name in enumerate(('ball', 'box')):
        rec = res['shapes'][name]
        assert set(rec) == today | new and saved['shapes'][name] == rec
        assert all(rec[x] == plain['shapes'][name][x] for x in ('gt', 'input_points'))
        v, f = res['meshes'][name]
        pts, nrm = clouds[name]
        assert rec['input_points'] == pts.shape[0] > npts
        sel = torch.arange(npts, device=dev()) * pts.shape[0] // npts
        if rec['faces']:
            want = RM.surface_scores((pts[sel] * ps, nrm[sel]), (v, f), n=npts, seed=4, thresholds=taus)
            assert rec['scores'] == want and math.isfinite(want['chamfer_l1']) and want['chamfer_l1'] > 0
        else:                                          # random weights may give no surface: the null path
            assert rec['scores'] is None
        field, b = res['fields'][name]
        assert b == k
        if name == 'ball':
            assert rec['iou'] is None and rec['iou_intersection'] is None and rec['iou_union'] is None
        else:
            want = RM.occupancy_iou(field, occ['points'], occ['occupancies'], ps, batch_index=b)
            assert (rec['iou'], rec['iou_intersection'], rec['iou_union']) == want
            assert 0 <= want[1] <= want[2] <= 1003
        print(name, 'faces', rec['faces'], 'scores', rec['scores'] and rec['scores']['chamfer_l1'], 'iou', rec['iou'])
