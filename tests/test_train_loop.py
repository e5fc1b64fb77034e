"""The training driver's loop logic (octfusion_amd/train.py) on the CPU: a stub takes the place of the stage step
(Trainer(step_fn=...)), so the sampler, the resume, the checkpoint rotation, the schedules and the loss read-back run
without a device.  The stub adds a function of the batch indices and the drawn `times` to a CPU parameter."""
import json
import math
import os

import pytest
import torch

from octfusion_amd import train as TN
from octfusion_amd.vae_training import poly_lr

N_NAMES = 11


def make_args(tmp_path, *extra):
    names = tmp_path / 'names.txt'
    if not names.exists():
        names.write_text(''.join('cat/%02d %d\n' % (i, i % 5) for i in range(N_NAMES)))
    return TN.parser().parse_args(['--model', 'lr', '--dataset-dir', str(tmp_path / 'data'), '--names', str(names),
                                   '--logs-dir', str(tmp_path / 'logs'), '--batch', '3', '--seed', '5'] + list(extra))


class Stub:
    """w += sum(idx) + 1000 * sum(times); records what it was given."""

    def __init__(self, nan_at=None):
        self.w = torch.zeros(2, dtype=torch.float64)
        self.seen = []
        self.nan_at = nan_at

    def __call__(self, tr, idx, times):
        self.seen.append((list(idx), times.clone()))
        self.w += float(sum(idx)) + 1000.0 * times.double().sum()
        loss = self.w.sum() * 1e-6
        if self.nan_at is not None and tr.iter == self.nan_at:
            loss = loss * float('nan')
        return {'loss': loss}

    def trainer(self, args, **kw):
        return TN.Trainer(args, step_fn=self, state={'w': self.w}, **kw)


def test_sampler_permutations_and_rank_shards():
    s = TN.InfSampler(N_NAMES, seed=3)
    first = s.batch(N_NAMES)
    second = s.batch(N_NAMES)
    assert sorted(first) == sorted(second) == list(range(N_NAMES))       # each name once per permutation
    assert first != second                                               # reshuffled when exhausted
    assert TN.InfSampler(N_NAMES, seed=3).batch(N_NAMES) == first        # seeded
    r0, r1 = TN.InfSampler(N_NAMES, seed=3, rank=0, world=2), TN.InfSampler(N_NAMES, seed=3, rank=1, world=2)
    per_rank = N_NAMES // 2
    a, b = r0.batch(per_rank), r1.batch(per_rank)
    assert not set(a) & set(b)
    assert len(set(a) | set(b)) == 2 * per_rank                          # the remainder is dropped, not padded
    assert sorted(a + b) == sorted(first[:2 * per_rank])                 # the same permutation, every 2nd position
    a2, b2 = r0.batch(per_rank), r1.batch(per_rank)                      # the next permutation, again disjoint
    assert not set(a2) & set(b2) and sorted(a2 + b2) == sorted(second[:2 * per_rank])
    with pytest.raises(ValueError):
        TN.InfSampler(1, world=2)


def test_resume_draws_what_the_uninterrupted_run_draws(tmp_path):
    straight = Stub()
    tr = straight.trainer(make_args(tmp_path, '--name', 'straight', '--epochs', '2'))
    assert tr.epoch_length == 3 and tr.total_iters == 6
    for _ in range(6):
        tr.step()
    # 3 steps + save + a fresh Trainer + load + 3 steps; the batch of 3 out of 11 crosses a permutation boundary
    args = make_args(tmp_path, '--name', 'split', '--epochs', '2')
    first = Stub()
    t1 = first.trainer(args)
    for _ in range(3):
        t1.step()
    path = t1.save('steps-latest')
    second = Stub()
    t2 = second.trainer(make_args(tmp_path, '--name', 'elsewhere', '--epochs', '2'))
    assert t2.iter == 0
    t2.load(path)
    assert t2.iter == 3 and torch.equal(second.w, first.w)
    for _ in range(3):
        t2.step()
    seen = first.seen + second.seen
    assert [i for i, _ in seen] == [i for i, _ in straight.seen]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for (_, a), (_, b) in zip(seen, straight.seen))           # identical `times` bits
    assert torch.equal(second.w, straight.w)
    # and the automatic resume: same logs dir and name, no --ckpt
    third = Stub()
    t3 = third.trainer(args)
    assert t3.iter == 3 and torch.equal(third.w, first.w)
    assert t3.sampler.batch(3) == straight.seen[3][0]


def test_run_resumes_and_appends(tmp_path):
    a = Stub()
    assert a.trainer(make_args(tmp_path, '--name', 'r', '--epochs', '1', '--print-freq', '2')).run() == 3
    b = Stub()
    tb = b.trainer(make_args(tmp_path, '--name', 'r', '--epochs', '2', '--print-freq', '2'))
    assert tb.iter == 3 and tb.run() == 6
    rows = [json.loads(ln) for ln in open(tmp_path / 'logs' / 'r' / 'loss.jsonl')]
    assert [r['iter'] for r in rows] == list(range(6))
    assert [r['epoch'] for r in rows] == [0, 0, 0, 1, 1, 1]
    assert all(set(r) == {'iter', 'epoch', 'lr', 'loss', 'seconds'} and math.isfinite(r['loss']) for r in rows)
    straight = Stub()
    straight.trainer(make_args(tmp_path, '--name', 's', '--epochs', '2')).run()
    assert torch.equal(b.w, straight.w)
    sd = torch.load(tmp_path / 'logs' / 'r' / 'ckpt' / 'df_steps-latest.pth', weights_only=True)
    assert sd['global_step'] == 6 and set(sd['train_state']) == {'sampler', 'times'}


def test_rotation_keeps_ckpt_num_numbered_files_and_latest(tmp_path):
    s = Stub()
    tr = s.trainer(make_args(tmp_path, '--name', 'rot', '--epochs', '4', '--save-steps-freq', '2',
                             '--save-latest-freq', '3', '--ckpt-num', '2'))
    assert tr.run() == 12
    files = sorted(os.listdir(tmp_path / 'logs' / 'rot' / 'ckpt'))
    assert files == ['df_steps-10.pth', 'df_steps-12.pth', 'df_steps-latest.pth']      # oldest deleted first
    assert torch.load(tmp_path / 'logs' / 'rot' / 'ckpt' / 'df_steps-latest.pth', weights_only=True)['global_step'] == 12


def test_schedules_closed_form():
    base, lo, E, W = 1e-4, 1e-6, 20, 4
    assert TN.cosine_lr(base, lo, 0, E, W) == base                       # before the warm-up epoch: the base rate
    assert TN.cosine_lr(base, lo, W, E, W) == pytest.approx(base, rel=1e-12)
    mid = W + (E - W) / 2
    assert TN.cosine_lr(base, lo, mid, E, W) == pytest.approx(lo + (base - lo) * 0.5, rel=1e-12)
    assert TN.cosine_lr(base, lo, E - 1, E, W) == pytest.approx(
        lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * (E - 1 - W) / (E - W))), rel=1e-12)
    assert TN.cosine_lr(base, lo, E, E, W) == pytest.approx(lo, rel=1e-9)
    assert TN.cosine_lr(base, lo, 5, 10, 0) == pytest.approx(lo + (base - lo) * 0.5, rel=1e-12)
    assert poly_lr(base, 0, E) == base
    assert poly_lr(base, E // 2, E) == pytest.approx(base * 0.5 ** 0.9, rel=1e-12)
    assert poly_lr(base, E - 1, E) == pytest.approx(base * (1 / E) ** 0.9, rel=1e-9)


def test_trainer_applies_the_schedule_per_epoch(tmp_path):
    s = Stub()
    tr = s.trainer(make_args(tmp_path, '--name', 'lr', '--epochs', '4', '--update-learning-rate', '--lr', '1e-3',
                             '--min-lr', '1e-5', '--warmup-epochs', '1', '--print-freq', '100'))
    tr.run()
    rows = [json.loads(ln) for ln in open(tmp_path / 'logs' / 'lr' / 'loss.jsonl')]
    assert [r['lr'] for r in rows] == [TN.cosine_lr(1e-3, 1e-5, r['iter'] // 3, 4, 1) for r in rows]
    assert rows[0]['lr'] == 1e-3 and rows[-1]['lr'] < rows[3]['lr']


def test_nan_loss_raises_at_the_print_boundary_before_any_save(tmp_path):
    s = Stub(nan_at=1)
    tr = s.trainer(make_args(tmp_path, '--name', 'nan', '--epochs', '4', '--print-freq', '4', '--save-latest-freq', '5'))
    with pytest.raises(FloatingPointError, match='iteration 1'):
        tr.run()
    assert tr.iter == 4                                                  # raised at the boundary, not at the step
    assert os.listdir(tmp_path / 'logs' / 'nan' / 'ckpt') == []
    rows = [json.loads(ln) for ln in open(tmp_path / 'logs' / 'nan' / 'loss.jsonl')]
    assert len(rows) == 4 and math.isnan(rows[1]['loss'])
    # a save that comes before the print boundary reads the losses first and refuses too
    s2 = Stub(nan_at=1)
    t2 = s2.trainer(make_args(tmp_path, '--name', 'nan2', '--epochs', '4', '--print-freq', '100',
                              '--save-latest-freq', '3'))
    with pytest.raises(FloatingPointError):
        t2.run()
    assert t2.iter == 3 and os.listdir(tmp_path / 'logs' / 'nan2' / 'ckpt') == []


def test_default_vae_geometry_of_the_named_configs():
    from octfusion_amd import configs
    for name in configs.CONFIGS:
        assert TN.default_vae_config(name, 'hr') == configs.vae_params(name)
        assert TN.default_vae_config(name, 'vae') == configs.vae_params(name)
    f = TN.default_vae_config('obja_uncond', 'feature')              # configs/vae_obja_train.yaml: depth 10, stop 8
    assert (f['depth'], f['depth_stop'], f['depth_out']) == (10, 8, 10)
    assert f['depth_stop'] == configs.CONFIGS['obja_uncond']['input_depth'][2]
    assert {k: v for k, v in f.items() if not k.startswith('depth')} == {
        k: v for k, v in configs.vae_params('obja_uncond').items() if not k.startswith('depth')}
    assert configs.vae_params('obja_uncond')['depth_stop'] == configs.CONFIGS['obja_uncond']['input_depth'][1]
