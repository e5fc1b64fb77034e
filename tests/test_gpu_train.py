"""GPU tests of the fused training step (training.lr_stage_step / hr_stage_step with fused=True: ofx_mse_grad + the
multi-tensor optimiser call) against the existing step, and of the training driver (octfusion_amd/train.py) end to end
on a two-shape dataset folder.

Bounds: the first-step loss of the fused step against the existing step's float uses the bound the existing tests use
against the oracle (tests/test_gpu_parity.py: 1e-4 relative for lr, 1e-3 for hr) -- both run the same forward, whose
atomics reorder sums run to run; the fused loss itself is an fp64 sum of the same fp32 differences.  The loss must fall
as those tests require (< 0.7x after 6 steps at 2e-3 for lr, < 0.9x at 1e-3 for hr)."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import common as C
import sdfdata_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def dev():
    return torch.device('cuda:0')


def load(module, keys):
    module.load_state_dict(C.fill_state_dict(keys), strict=True)
    return module.to(dev()).eval()


def union_cfg():
    h, l = C.TINY_HR_CFG, C.TINY_LR_CFG
    return dict(image_size=[8, 32], input_depth=[3, 5], unet_type=['lr', 'hr'], full_depth=3, input_channels=[8, 3],
                out_channels=[8, 3], model_channels=[l['model_channels'], h['model_channels']],
                num_res_blocks=[[1, 1, 1], h['num_res_blocks']], attention_resolutions=[2, 4],
                channel_mult=[l['channel_mult'], h['channel_mult']], num_heads=4, use_checkpoint=False, dims=3)


def test_fused_lr_stage_step(golden):
    from octfusion_amd import graph_unet_lr as LR, training as TR
    keys = golden('g_dense')['lr']['keys']
    B, S = 2, 8
    split = C.random_split_small(B, 3, 9, p=0.4).to(dev())
    g = torch.Generator().manual_seed(11)
    times = [torch.rand(B, generator=g) for _ in range(6)]                       # on the CPU: no device->host copy
    noises = [torch.randn(B, 8, S, S, S, generator=g).to(dev()) for _ in range(6)]
    runs = {}
    for fused in (False, True):
        net = load(LR.UNet3DModel(**C.TINY_LR_CFG), keys)
        ema = copy.deepcopy(net)
        opt = TR.AdamW(dict(net.named_parameters()), lr=2e-3)
        out = [TR.lr_stage_step(net, opt, split, t, nz, ema=ema, ema_rate=0.9, fused=fused) for t, nz in zip(times, noises)]
        runs[fused] = (out, net, ema)
    plain, fused = runs[False][0], runs[True][0]
    assert all(isinstance(v, float) for v in plain)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 and v.dtype == torch.float64 for v in fused)
    fused = [float(v) for v in fused]
    print('lr losses: plain %s, fused %s' % (plain, fused))
    assert abs(fused[0] - plain[0]) <= 1e-4 * plain[0], (fused[0], plain[0])
    assert fused[-1] < 0.7 * fused[0] and plain[-1] < 0.7 * plain[0]
    # the EMA folded into the optimiser call moved and stayed finite (its bits against ema_update:
    # tests/test_gpu_train_kernels.py)
    ema_f, net_f = runs[True][2], runs[True][1]
    assert all(bool(torch.isfinite(p).all()) for p in ema_f.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(ema_f.parameters(), net_f.parameters()))


def test_fused_hr_stage_step_and_frozen_nested_net(golden):
    from octfusion_amd import graph_unet_union as U, training as TR
    from octfusion_amd.dual_octree import DualOctree
    from octfusion_amd.octree import split2octree_small
    G = golden('g_unet')
    r = G['uncond']
    doc = DualOctree(split2octree_small(G['split_small'].to(dev()), 5, 3))
    doc.post_processing_for_docnn()
    N = doc.total_num
    codes, noise = C.rand_input('hrt_codes', N, 3).to(dev()), C.rand_input('hrt_noise', N, 3).to(dev())
    times = torch.tensor([0.35, 0.8])
    runs = {}
    for fused in (False, True):
        net = load(U.UNet3DModel(stage_flag='hr', **union_cfg()), r['keys'])
        ema = copy.deepcopy(net)
        before = {k: v.clone() for k, v in net.unet_lr.state_dict().items()}
        ema_before = {k: v.clone() for k, v in ema.state_dict().items()}
        opt = TR.AdamW(TR.trainable_parameters(net, 'hr'), lr=1e-3)                # the driver's optimiser: own stage only
        out = [TR.hr_stage_step(net, opt, codes, doc, 5, times, noise, ema=ema, ema_rate=0.9, fused=fused)
               for _ in range(6)]
        for k, v in net.unet_lr.state_dict().items():
            assert torch.equal(v, before[k]), 'nested lr parameter %s changed (fused=%s)' % (k, fused)
        runs[fused] = ([float(v) for v in out], net, ema, ema_before)
    plain, fused = runs[False][0], runs[True][0]
    print('hr losses: plain %s, fused %s' % (plain, fused))
    assert abs(fused[0] - plain[0]) <= 1e-3 * plain[0], (fused[0], plain[0])
    assert fused[-1] < 0.9 * fused[0] and plain[-1] < 0.9 * plain[0]
    # the EMA runs over the whole net, frozen stage included (its value there: e * beta + (1 - beta) * e six times,
    # the same kernel arithmetic in both runs, so the two EMA copies of the frozen stage are equal bits)
    ema_p, ema_f = runs[False][2], runs[True][2]
    for (k, a), b in zip(ema_p.unet_lr.state_dict().items(), ema_f.unet_lr.state_dict().values()):
        assert torch.equal(a, b), k
    moved = [k for k, v in ema_f.unet_hr.state_dict().items() if not torch.equal(v, runs[True][3]['unet_hr.' + k])]
    assert moved


# ---------------------------------------------------------------------------------------------------- the driver
VAE_CFG = dict(depth=4, channel_in=4, nout=4, full_depth=2, depth_stop=3, depth_out=4, resblk_type='basic',
               resblk_num=2, code_channel=16, embed_dim=3)


def sphere_cloud(n, seed, radius=0.55, centre=(0.07, -0.05, 0.03)):
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return nrm * radius + torch.tensor(centre), nrm


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """The two-shape dataset folder of tests/test_gpu_sdfdata.py::test_dataset_folder_to_training_step."""
    from octfusion_amd import dataset as D
    root = tmp_path_factory.mktemp('train')
    S, names, radii = 32, ['cat/a', 'cat/b'], [0.55, 0.4]
    sdf_dir, data_dir = root / 'sdf', root / 'dataset'
    for name, r in zip(names, radii):
        (sdf_dir / 'cat').mkdir(parents=True, exist_ok=True)
        (data_dir / name).mkdir(parents=True)
        np.save(str(sdf_dir / (name + '.npy')), O.sphere_lattice(S, radius=r))
        pts, nrm = sphere_cloud(3000, 1, radius=r)
        np.savez(str(data_dir / name / 'pointcloud.npz'), points=(pts * 0.5).numpy().astype(np.float16),
                 normals=nrm.numpy().astype(np.float16))
    D.main(['--sdf-dir', str(sdf_dir), '--dataset-dir', str(data_dir), '--depth', '4', '--full-depth', '2'])
    (root / 'names.txt').write_text('cat/a 0\ncat/b 1\n')
    return root


def argv(folder, model, name, epochs, *extra):
    return ['--model', model, '--dataset-dir', str(folder / 'dataset'), '--names', str(folder / 'names.txt'),
            '--logs-dir', str(folder / 'logs'), '--name', name, '--epochs', str(epochs), '--batch', '2', '--seed', '3',
            '--point-sample-num', '300', '--print-freq', '3'] + list(extra)


def rows_of(folder, name):
    return [json.loads(ln) for ln in open(folder / 'logs' / name / 'loss.jsonl')]


def test_driver_trains_the_vae_and_resumes(folder):
    from octfusion_amd import checkpoint as CK, train as TN
    from octfusion_amd.graph_vae import GraphVAE
    assert TN.main(argv(folder, 'vae', 'v', 4, '--lr', '1e-4'), config=VAE_CFG) == 4       # 2 names / batch 2: 1 step an epoch
    latest = folder / 'logs' / 'v' / 'ckpt' / 'vae_steps-latest.pth'
    assert latest.exists()
    vae = CK.load_vae(str(latest), GraphVAE(**VAE_CFG))                                    # strict
    assert all(bool(torch.isfinite(p).all()) for p in vae.parameters())
    sd = torch.load(str(latest), weights_only=True)
    assert {'autoencoder', 'opt', 'global_step', 'train_state'} <= set(sd) and sd['global_step'] == 4
    assert sd['opt']['step'] == 4
    rows = rows_of(folder, 'v')
    assert [r['iter'] for r in rows] == [0, 1, 2, 3]
    assert all(math.isfinite(v) for r in rows for v in r.values())
    assert {'loss', 'kl_loss', 'sdf_loss_4', 'grad_loss_4', 'loss_4'} <= set(rows[0])
    assert [r['lr'] for r in rows] == [1e-4 * (1 - e / 4) ** 0.9 for e in range(4)]        # poly_lr per epoch
    # the same arguments with more epochs: resumes at global_step and appends
    assert TN.main(argv(folder, 'vae', 'v', 6, '--lr', '1e-4'), config=VAE_CFG) == 6
    rows = rows_of(folder, 'v')
    assert [r['iter'] for r in rows] == [0, 1, 2, 3, 4, 5]
    sd = torch.load(str(latest), weights_only=True)
    assert sd['global_step'] == 6 and sd['opt']['step'] == 6


def test_driver_trains_the_lr_stage_and_resumes(folder):
    from octfusion_amd import checkpoint as CK, train as TN, training as TR
    from octfusion_amd.graph_unet_union import UNet3DModel
    cfg = dict(union_cfg(), df_type=['x0', 'eps'])
    args = TN.parser().parse_args(argv(folder, 'lr', 'l', 4, '--lr', '1e-3', '--ema-rate', '0.9'))
    tr = TN.Trainer(args, config=cfg)
    assert tr.run() == 4
    latest = folder / 'logs' / 'l' / 'ckpt' / 'df_steps-latest.pth'
    rows = rows_of(folder, 'l')
    assert [r['iter'] for r in rows] == [0, 1, 2, 3] and all(math.isfinite(r['loss']) and r['loss'] > 0 for r in rows)
    raw = torch.load(str(latest), weights_only=True)
    assert set(raw) == {'df_unet_lr', 'ema_df_unet_lr', 'opt', 'global_step', 'train_state'}
    assert set(raw['train_state']) == {'sampler', 'times', 'device_rng'}
    # a fresh net, EMA and optimiser read it back
    kw = {k: v for k, v in cfg.items() if k != 'df_type'}
    fresh, fresh_ema = UNet3DModel(stage_flag='lr', **kw).to(dev()), UNet3DModel(stage_flag='lr', **kw).to(dev())
    opt = TR.AdamW(fresh.unet_lr.named_parameters(), lr=1e-3)
    assert CK.load_ckpt(str(latest), fresh, fresh_ema, opt=opt) == 4
    for (k, a), b in zip(tr.stage.net.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(a, b), k
    for (k, a), b in zip(tr.stage.ema.state_dict().items(), fresh_ema.state_dict().values()):
        assert torch.equal(a, b), k
    assert any(not torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), fresh_ema.state_dict().values()))
    assert opt.step_count == tr.stage.opt.step_count == 4
    for k, (m, v) in tr.stage.opt.state.items():
        assert torch.equal(m, opt.state[k][0]) and torch.equal(v, opt.state[k][1]), k
    assert any(bool(m.any()) for m, _ in opt.state.values())
    # resume: a second trainer with the same arguments and more epochs starts at step 4 with the first one's weights
    t2 = TN.Trainer(TN.parser().parse_args(argv(folder, 'lr', 'l', 6, '--lr', '1e-3', '--ema-rate', '0.9')), config=cfg)
    assert t2.iter == 4 and t2.stage.opt.step_count == 4
    for (k, a), b in zip(tr.stage.net.state_dict().items(), t2.stage.net.state_dict().values()):
        assert torch.equal(a, b), k
    assert t2.run() == 6
    assert [r['iter'] for r in rows_of(folder, 'l')] == [0, 1, 2, 3, 4, 5]
    assert os.path.exists(latest) and torch.load(str(latest), weights_only=True)['global_step'] == 6


# ------------------------------------------------------------------------------- the sparse stages of the driver
CFG3 = dict(image_size=[8, 32, 128], input_depth=[3, 5, 7], unet_type=['lr', 'hr', 'feature'], full_depth=3,
            input_channels=[8, 8, 3], out_channels=[8, 8, 3], model_channels=[16, 32, 32],
            num_res_blocks=[[1, 1, 1], [1, 1, 0], [1, 1, 1]], attention_resolutions=[2, 4],
            channel_mult=[[1, 2, 4], [1, 2, 4], [1, 2, 4]], num_heads=4, use_checkpoint=False, dims=3,
            df_type=['x0', 'x0', 'x0'])


def tiny_vae(folder, name, depth, stop):
    """A GraphVAE geometry (depth / depth_stop) with seeded random weights, written as a checkpoint file."""
    from octfusion_amd import synthetic
    from octfusion_amd.graph_vae import GraphVAE
    cfg = dict(VAE_CFG, depth=depth, full_depth=3, depth_stop=stop, depth_out=depth)
    path = folder / (name + '.pth')
    torch.save({'autoencoder': synthetic.random_state_dict(GraphVAE(**cfg))}, str(path))
    return cfg, str(path)


def pretrain(folder, name, cfg, stage):
    """df_*.pth of the stages up to `stage` with filled weights; returns (path, the net)."""
    from octfusion_amd import checkpoint as CK
    from octfusion_amd.graph_unet_union import UNet3DModel
    net = UNet3DModel(stage_flag=stage, **{k: v for k, v in cfg.items() if k != 'df_type'})
    net.load_state_dict(C.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()]))
    path = str(folder / (name + '.pth'))
    CK.save_ckpt(path, net, net, 0, stage_flag=stage)
    return path, net


def run_sparse(folder, model, name, cfg, vae_cfg, frozen, *extra):
    """Two steps of a sparse stage through the Trainer; the frozen earlier stages must stay the pretrain's bits."""
    from octfusion_amd import train as TN
    ckpt, pre = pretrain(folder, name + '_pre', cfg, frozen[-1])
    args = TN.parser().parse_args(argv(folder, model, name, 2, '--lr', '1e-3', '--ema-rate', '0.9', '--pretrain-ckpt',
                                       ckpt, *extra))
    tr = TN.Trainer(args, config=cfg, vae_config=vae_cfg)
    own = getattr(tr.stage.net, 'unet_' + model)
    before = {k: v.clone() for k, v in own.state_dict().items()}
    assert tr.run() == 2
    rows = rows_of(folder, name)
    assert [r['iter'] for r in rows] == [0, 1] and all(math.isfinite(r['loss']) and r['loss'] > 0 for r in rows)
    for kind in frozen:
        want = getattr(pre, 'unet_' + kind).state_dict()
        for k, v in getattr(tr.stage.net, 'unet_' + kind).state_dict().items():
            assert torch.equal(v.cpu(), want[k]), (kind, k)
    assert any(not torch.equal(v, before[k]) for k, v in own.state_dict().items())
    raw = torch.load(str(folder / 'logs' / name / 'ckpt' / 'df_steps-latest.pth'), weights_only=True)
    assert 'df_unet_' + model in raw and 'ema_df_unet_' + model in raw and raw['global_step'] == 2
    return tr


def test_driver_runs_the_hr_stage_on_vae_codes(folder):
    cfg = dict(union_cfg(), df_type=['x0', 'eps'])
    vae_cfg, vae_path = tiny_vae(folder, 'vae65', 6, 5)
    run_sparse(folder, 'hr', 'h2', cfg, vae_cfg, ['lr'], '--vae', vae_path)
    from octfusion_amd import train as TN
    with pytest.raises(ValueError, match='--vae is required'):
        TN.Trainer(TN.parser().parse_args(argv(folder, 'hr', 'h2x', 2)), config=cfg, vae_config=vae_cfg)
    bad_cfg, bad_path = tiny_vae(folder, 'vae64', 6, 4)
    with pytest.raises(ValueError, match='codes live at depth 4'):
        TN.Trainer(TN.parser().parse_args(argv(folder, 'hr', 'h2y', 2, '--vae', bad_path)), config=cfg,
                   vae_config=bad_cfg)


def test_driver_runs_the_three_stage_hr_and_feature_stages(folder):
    from octfusion_amd import train as TN
    from octfusion_amd.dual_octree import DualOctree
    from octfusion_amd.octree import build_octree_batch, octree2split_large
    tr = run_sparse(folder, 'hr', 'h3', CFG3, None, ['lr'])
    assert tr.stage.vae is None and tr.stage.data.flags['depth'] == 7
    # the zero-padded split: rows of the depth-5 graph = leaves of depths 3 and 4, then every depth-5 node
    clouds = [s['points'].to(dev()) for s in tr.stage.data.samples([0, 1])]
    octree = build_octree_batch(clouds, 7, 3)
    doc = DualOctree(octree)
    data = TN.padded_split_large(octree, doc, 5)
    split = octree2split_large(octree, 5)
    lead = int(doc.lnum[3] + doc.lnum[4])
    assert lead > 0 and data.shape == (lead + int(doc.nnum[5]), 8) and split.shape[0] == int(doc.nnum[5])
    assert not data[:lead].any() and torch.equal(data[lead:], split)
    assert set(split.unique().tolist()) == {-1.0, 1.0}
    vae_cfg, vae_path = tiny_vae(folder, 'vae87', 8, 7)
    run_sparse(folder, 'feature', 'f3', CFG3, vae_cfg, ['lr', 'hr'], '--vae', vae_path)
