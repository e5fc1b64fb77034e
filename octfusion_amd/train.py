"""Training driver: dataset folder in, checkpoints out.

The reference's train.py:33-130 plus its model wrappers' optimizer_initialize / set_input / forward / save
(models/octfusion_model_vae.py, octfusion_model_union.py, octfusion_model_union_3t.py), for the four things it trains:

  --model vae      ReadFile -> TransformShape -> collate -> to_device_batch -> vae_training.vae_stage_step
  --model lr       point clouds -> octree at input_depth[1] -> split codes -> training.lr_stage_step on unet_lr
  --model hr       2-stage configs: the VAE's codes (extract_code) -> hr_stage_step(stage='hr');
                   the 3-stage config: octree2split_large on the depth-6 graph rows (zero rows for the leaves of the
                   shallower depths, the split in the last nnum rows) -> hr_stage_step(stage='hr')
  --model feature  the VAE's codes at the large depth -> hr_stage_step(stage='feature')

Only the stage's own net is trained; earlier stages come from --pretrain-ckpt / --ckpt with the reference's
load_options and stay frozen; the EMA net is a deep copy and its update runs over the whole net.

    python -m octfusion_amd.train --model lr --config snet_uncond --dataset-dir D --names FILE --logs-dir L --name N
        --epochs E --batch B --seed S [--vae PATH] [--no-fused]

What differs from the reference loop:
  * Learning rate: constant --lr, or with --update-learning-rate the reference's half-cosine per epoch
    (base_model.py:81-91).  The reference also builds a StepLR(1000, 0.9) and never steps it: not imitated.  Its
    "warm-up" holds the base rate until --warmup-epochs (there is no ramp); kept.  The VAE follows
    vae_training.poly_lr per epoch.
  * Sampler: the reference's InfSampler (an endless stream of permutations of the name list) drawn from a CPU
    generator seeded with --seed; rank r takes every world-th position of a permutation.  The reference's
    DistributedSampler pads the list to a multiple of the world size; here the remainder of a permutation is DROPPED,
    so ranks never see a shape twice in one permutation and a permutation yields world * floor(N / world) names.
  * No host wait inside a step: `times` come from a CPU generator, the losses stay on the device and are read once
    every --print-freq steps (one JSON line per step in <logs>/<name>/loss.jsonl).  A non-finite loss raises there,
    and before any save; the reference asserts every step.
  * Checkpoints carry one more key, 'train_state' (sampler position, the generator states that draw the batches, the
    `times` and the noise), which the reference's loader ignores; with it a resumed run draws what the uninterrupted run
    would have drawn.  Rotation keeps --ckpt-num numbered files, oldest deleted first; "latest" is never counted.
  * The periodic sample / inference preview inside the loop and tensorboard are not here: generate.py and
    reconstruct.py run from the saved checkpoint.
  * Under torchrun: dist.init(), rank 0 writes the files, AdamW.sync_ aligns the ranks at construction and the
    gradients are averaged per step.  More than one rank has not run on hardware.
"""
import argparse
import copy
import json
import math
import os
import re
import time

import torch

from . import configs

MODELS = ('vae', 'lr', 'hr', 'feature')


# ---------------------------------------------------------------------------------------------------- schedules
def cosine_lr(base_lr, min_lr, epoch, epochs, warmup_epochs=0):
    """base_model.py:81-91: half-cycle cosine from base_lr to min_lr over the epochs after warmup_epochs; before
    them the rate is left at base_lr (the reference has no ramp)."""
    if epoch < warmup_epochs:
        return base_lr
    return min_lr + (base_lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch - warmup_epochs) /
                                                               (epochs - warmup_epochs)))


# ---------------------------------------------------------------------------------------------------- sampler
class InfSampler:
    """datasets/sampler.py:12-40: an endless stream of permutations of range(n), reshuffled when exhausted.  The
    permutations come from a CPU generator; rank r of `world` takes positions r, r + world, ... of each, and the
    n mod world names at the end of a permutation are dropped (not padded), so the ranks' draws are disjoint."""

    def __init__(self, n, seed=0, rank=0, world=1):
        if n < world:
            raise ValueError('InfSampler: %d names for %d ranks' % (n, world))
        self.n, self.rank, self.world = int(n), int(rank), int(world)
        self.usable = (self.n // self.world) * self.world
        self.gen = torch.Generator()
        self.gen.manual_seed(int(seed))
        self._shuffle()

    def _shuffle(self):
        self._before = self.gen.get_state()          # a permutation is re-drawn from this state on resume
        self.perm = torch.randperm(self.n, generator=self.gen).tolist()
        self.pos = 0

    def next(self):
        if self.pos >= self.usable:
            self._shuffle()
        i = self.perm[self.pos + self.rank]
        self.pos += self.world
        return i

    def batch(self, size):
        return [self.next() for _ in range(size)]

    def state_dict(self):
        return {'gen': self._before.clone(), 'pos': self.pos, 'n': self.n, 'world': self.world}

    def load_state_dict(self, sd):
        if int(sd['n']) != self.n or int(sd['world']) != self.world:
            raise ValueError('sampler state of %d names / %d ranks, this run has %d / %d'
                             % (sd['n'], sd['world'], self.n, self.world))
        self.gen.set_state(sd['gen'])
        self._shuffle()
        self.pos = int(sd['pos'])


def read_names(path):
    """The name list: one shape per line, `<name> [<label>]` -> (names, labels or None)."""
    names, labels = [], []
    with open(path) as fh:
        for ln in fh:
            w = ln.split()
            if w:
                names.append(w[0])
                labels.append(int(w[1]) if len(w) > 1 else None)
    return names, (labels if names and all(v is not None for v in labels) else None)


# ---------------------------------------------------------------------------------------------------- stages
def _device():
    return torch.device('cuda', torch.cuda.current_device())


class _Data:
    """ReadFile + TransformShape of one stage.  A shape's random choices are keyed by the visit (step, rank, slot), not
    by the shape: every visit draws afresh and a resumed run draws the same."""

    def __init__(self, tr, depth, full_depth, load_sdf):
        from . import dataset as D
        self.D = D
        a = tr.args
        self.flags = {'depth': depth, 'full_depth': full_depth, 'point_scale': a.point_scale,
                      'point_sample_num': a.point_sample_num, 'load_pointcloud': True, 'load_sdf': load_sdf,
                      'load_occu': False, 'sample_surf_points': False}
        self.read, self.transform = D.ReadFile(self.flags), D.TransformShape(self.flags, seed=a.seed)
        self.tr = tr

    def samples(self, idx):
        tr = self.tr
        visit = (tr.iter * tr.world + tr.rank) * len(idx)
        return [self.transform(self.read(os.path.join(tr.args.dataset_dir, tr.names[i])), visit + j)
                for j, i in enumerate(idx)]


def padded_split_large(octree, doctree, small_depth):
    """octfusion_model_union_3t.py:136-139: the depth-`small_depth` split codes on the rows of the dual graph of that
    depth -- zero rows for the leaves of the shallower depths, octree2split_large in the last nnum[small_depth] rows."""
    from .octree import octree2split_large
    split = octree2split_large(octree, small_depth)
    rows = doctree.batch_id(small_depth).shape[0]
    data = torch.zeros(rows, split.shape[1], dtype=torch.float32, device=split.device)
    data[rows - split.shape[0]:] = split
    return data


def default_vae_config(config, model):
    """GraphVAE keyword arguments of a named config.  The feature stage trains on codes at its own depth, so its VAE is
    the reference's configs/vae_obja_train.yaml geometry: two levels above input_depth[-1], stopping at it."""
    cfg = configs.vae_params(config)
    if model == 'feature':
        d = configs.CONFIGS[config]['input_depth'][-1]
        cfg.update(depth=d + 2, depth_stop=d, depth_out=d + 2)
    return cfg


class VaeStage:
    """octfusion_model_vae.py: the GraphVAE on (point cloud, SDF samples) batches."""
    prefix = 'vae'
    draws_times = False

    def __init__(self, tr, cfg):
        from . import training as T
        from .graph_vae import GraphVAE
        a = tr.args
        self.tr = tr
        self.vae = GraphVAE(**cfg).to(_device())
        self.opt = T.AdamW(self.vae.named_parameters(), lr=a.lr)
        self.data = _Data(tr, cfg['depth'], cfg['full_depth'], load_sdf=True)

    def lr(self, epoch):
        from .vae_training import poly_lr
        return poly_lr(self.tr.args.lr, epoch, self.tr.args.epochs)

    def step(self, idx, times):
        from .vae_training import vae_stage_step
        D = self.data.D
        args = D.to_device_batch(D.collate(self.data.samples(idx)), self.data.flags)
        losses = vae_stage_step(self.vae, self.opt, fused=self.tr.args.fused, **args)
        return {k: v for k, v in losses.items() if 'loss' in k}

    def save(self, path, global_step, train_state):
        torch.save({'autoencoder': self.vae.state_dict(), 'opt': self.opt.state_dict(), 'global_step': global_step,
                    'train_state': train_state}, path)

    def load(self, path, resume):
        from . import checkpoint as CK
        sd = CK._read(path)
        self.vae.load_state_dict(CK.vae_state_dict(sd), strict=True)
        if resume and isinstance(sd.get('opt'), dict) and 'state' in sd['opt']:
            self.opt.load_state_dict(sd['opt'])
        return sd


class DiffusionStage:
    """octfusion_model_union.py / octfusion_model_union_3t.py for one stage_flag."""
    prefix = 'df'
    draws_times = True

    def __init__(self, tr, cfg, vae_cfg):
        from . import checkpoint as CK, training as T
        from .graph_unet_union import UNet3DModel
        a = tr.args
        self.tr, self.cfg, self.stage = tr, cfg, a.model
        kinds = list(cfg['unet_type'])
        if self.stage not in kinds:
            raise ValueError('this config has no %r stage (stages: %s)' % (self.stage, kinds))
        self.si = kinds.index(self.stage)
        self.df_type = cfg['df_type'][self.si]
        if self.stage == 'lr' and self.df_type != 'x0':
            raise ValueError('the lr stage regresses x0 (training.lr_stage_step)')
        kw = {k: v for k, v in cfg.items() if k not in ('df_type', 'stage_flag')}
        dev = _device()
        self.net = UNet3DModel(stage_flag=self.stage, **kw).to(dev)
        self.three = len(kinds) == 3
        # earlier stages: --pretrain-ckpt with the reference's load_options (union.py:127-128, union_3t.py:80-85)
        self.ema = copy.deepcopy(self.net)
        if a.pretrain_ckpt:
            CK.load_ckpt(a.pretrain_ckpt, self.net, self.ema,
                         load_options=['unet_' + k for k in kinds[:max(self.si, 1)]])
        if self.stage == 'lr':                 # lr_stage_step names the gradients as unet_lr's own state_dict does
            self.opt = T.AdamW(self.net.unet_lr.named_parameters(), lr=a.lr)
        else:
            self.opt = T.AdamW(T.trainable_parameters(self.net, self.stage), lr=a.lr)
        self.uses_vae = self.stage == 'feature' or (self.stage == 'hr' and not self.three)
        self.vae = None
        if self.uses_vae:
            from .graph_vae import GraphVAE
            if not a.vae or vae_cfg is None:
                raise ValueError('--model %s trains on the codes of a trained GraphVAE: --vae is required' % self.stage)
            self.vae = CK.load_vae(a.vae, GraphVAE(**vae_cfg)).to(dev)
            want = cfg['input_depth'][self.si]
            if self.vae.depth_stop != want:
                raise ValueError('the %s stage runs on depth-%d rows, this VAE\'s codes live at depth %d'
                                 % (self.stage, want, self.vae.depth_stop))
        if self.stage == 'lr':
            depth = cfg['input_depth'][1] if len(kinds) > 1 else cfg['full_depth'] + 1
        else:
            depth = vae_cfg['depth'] if vae_cfg is not None else cfg['input_depth'][-1]
        self.small_depth = cfg['input_depth'][1] if len(kinds) > 1 else None
        self.data = _Data(tr, depth, cfg['full_depth'], load_sdf=False)
        self.labels = None
        if cfg.get('num_classes') is not None:
            if tr.labels is None:
                raise ValueError('a conditional config needs the label in the second column of --names')
            self.labels = torch.tensor(tr.labels, dtype=torch.int64)

    def lr(self, epoch):
        a = self.tr.args
        if not a.update_learning_rate:
            return a.lr
        return cosine_lr(a.lr, a.min_lr, epoch, a.epochs, a.warmup_epochs)

    @torch.no_grad()
    def step(self, idx, times):
        from . import training as T
        from .dual_octree import DualOctree
        from .octree import build_octree_batch, octree2split_small
        a = self.tr.args
        dev = _device()
        clouds = [s['points'].to(dev) for s in self.data.samples(idx)]
        octree = build_octree_batch(clouds, self.data.flags['depth'], self.cfg['full_depth'])
        label = self.labels[idx].to(dev) if self.labels is not None else None
        kw = dict(times=times, label=label, ema_rate=a.ema_rate, fused=a.fused)
        if self.stage == 'lr':
            split = octree2split_small(octree, self.cfg['full_depth'])
            loss = T.lr_stage_step(self.net.unet_lr, self.opt, split, ema=self.ema.unet_lr, **kw)
        elif self.uses_vae:
            codes, doctree = self.vae.extract_code(octree)
            loss = T.hr_stage_step(self.net, self.opt, codes, doctree, self.vae.depth_stop, ema=self.ema,
                                   stage=self.stage, df_type=self.df_type, **kw)
        else:                                   # 3-stage hr: octfusion_model_union_3t.py:132-143
            doctree = DualOctree(octree)
            data = padded_split_large(octree, doctree, self.small_depth)
            loss = T.hr_stage_step(self.net, self.opt, data, doctree, self.small_depth, ema=self.ema, stage='hr',
                                   df_type=self.df_type, **kw)
        return {'loss': loss if torch.is_tensor(loss) else torch.tensor(loss, dtype=torch.float64)}

    def save(self, path, global_step, train_state):
        from . import checkpoint as CK
        CK.save_ckpt(path, self.net, self.ema, global_step, stage_flag=self.stage, opt_state=self.opt.state_dict(),
                     extra={'train_state': train_state})

    def load(self, path, resume):
        from . import checkpoint as CK
        sd = CK._read(path)
        own = ['unet_' + k for k in list(self.cfg['unet_type'])[:self.si + 1]]
        CK.load_ckpt(sd, self.net, self.ema, load_options=own, opt=self.opt if resume else None)
        return sd


class StubStage:
    """A stage made of a caller's function and tensors: Trainer(args, step_fn=f, state={'w': tensor}).  `f(trainer,
    indices, times)` returns {name: 0-d tensor}; the tensors of `state` travel in the checkpoint under 'stub'."""
    prefix = 'df'
    draws_times = True

    def __init__(self, tr, step_fn, state):
        self.tr, self.fn, self.state = tr, step_fn, dict(state or {})

    def lr(self, epoch):
        a = self.tr.args
        return cosine_lr(a.lr, a.min_lr, epoch, a.epochs, a.warmup_epochs) if a.update_learning_rate else a.lr

    def step(self, idx, times):
        return self.fn(self.tr, idx, times)

    def save(self, path, global_step, train_state):
        torch.save({'stub': {k: v.detach().cpu().clone() for k, v in self.state.items()}, 'global_step': global_step,
                    'train_state': train_state}, path)

    def load(self, path, resume):
        from . import checkpoint as CK
        sd = CK._read(path)
        for k, v in sd.get('stub', {}).items():
            self.state[k].copy_(v)
        return sd


# ---------------------------------------------------------------------------------------------------- the loop
class Trainer:
    """train.py:33-130.  args: the namespace of parser(); config / vae_config: names in configs.CONFIGS (the command
    line) or the dicts themselves (UNet3DModel's list-valued parameters with 'df_type'; GraphVAE's keyword arguments).
    step_fn / state: a stub in place of the stage (StubStage) -- the loop, sampler, schedules and checkpoints then run
    without a device."""

    def __init__(self, args, config=None, vae_config=None, step_fn=None, state=None, rank=0, world=1):
        self.args, self.rank, self.world = args, int(rank), int(world)
        self.names, self.labels = read_names(args.names)
        self.dir = os.path.join(args.logs_dir, args.name)
        self.ckpt_dir = os.path.join(self.dir, 'ckpt')
        self.epoch_length = max(1, (len(self.names) // self.world) // args.batch)
        self.total_iters = self.epoch_length * args.epochs
        self.iter = 0
        self.sampler = InfSampler(len(self.names), args.seed, self.rank, self.world)
        self.gen_times = torch.Generator()
        self.gen_times.manual_seed(args.seed * 7919 + 1 + self.rank)
        self.pending = []
        self._window_t0 = None
        self.on_device = step_fn is None
        if step_fn is not None:
            self.stage = StubStage(self, step_fn, state)
        else:
            from . import _lib
            _lib.require_device()
            config = config if config is not None else args.config
            if vae_config is None and isinstance(config, str):
                vae_config = default_vae_config(config, args.model)
            torch.manual_seed(args.seed)                       # the nets' own initialisation
            torch.cuda.manual_seed(args.seed * 7919 + 2 + self.rank)   # the device generator draws the noise
            if args.model == 'vae':
                cfg = configs.vae_params(config) if isinstance(config, str) else dict(config)
                self.stage = VaeStage(self, cfg)
            else:
                cfg = configs.CONFIGS[config] if isinstance(config, str) else config
                self.stage = DiffusionStage(self, cfg, vae_config)
        if self.rank == 0:
            os.makedirs(self.ckpt_dir, exist_ok=True)
        ckpt = args.ckpt
        latest = self.path('steps-latest')
        if ckpt is None and os.path.exists(latest):            # resume, as the reference does (union.py:150-151)
            ckpt = latest
        if ckpt is not None:
            self.load(ckpt)

    # ---- files
    def path(self, label):
        return os.path.join(self.ckpt_dir, '%s_%s.pth' % (self.stage.prefix, label))

    def train_state(self):
        st = {'sampler': self.sampler.state_dict(), 'times': self.gen_times.get_state()}
        if self.on_device:
            st['device_rng'] = torch.cuda.get_rng_state(_device())
        return st

    def save(self, label):
        """<prefix>_<label>.pth (rank 0).  The pending losses are read first: a non-finite one raises before the file
        is written.  Numbered files beyond --ckpt-num are deleted oldest first; "latest" is never counted."""
        self.flush()
        if self.rank != 0:
            return None
        path = self.path(label)
        tmp = path + '.tmp'
        self.stage.save(tmp, self.iter, self.train_state())
        os.replace(tmp, path)
        pat = re.compile(r'^%s_steps-(\d+)\.pth$' % self.stage.prefix)
        numbered = sorted((int(m.group(1)), f) for f in os.listdir(self.ckpt_dir) for m in [pat.match(f)] if m)
        for _, f in numbered[:max(0, len(numbered) - self.args.ckpt_num)]:
            os.remove(os.path.join(self.ckpt_dir, f))
        return path

    def load(self, path):
        """Weights, and from a file of this driver the optimiser, the step count and the state of every generator."""
        sd = self.stage.load(path, resume=True)
        st = sd.get('train_state')
        if st is None:                                         # a reference checkpoint: weights only
            return
        self.iter = int(sd.get('global_step') or 0)
        self.sampler.load_state_dict(st['sampler'])
        self.gen_times.set_state(st['times'])
        if self.on_device and 'device_rng' in st:
            torch.cuda.set_rng_state(st['device_rng'], _device())

    # ---- one step
    def step(self, idx=None):
        """One optimisation step on the next batch of the sampler (or on `idx`).  Nothing is read back: the losses
        join self.pending as device tensors."""
        a = self.args
        if self._window_t0 is None:
            self._window_t0 = time.perf_counter()
        if idx is None:
            idx = self.sampler.batch(a.batch)
        epoch = self.iter // self.epoch_length
        lr = self.stage.lr(epoch)
        if hasattr(self.stage, 'opt'):
            self.stage.opt.lr = lr
        times = torch.rand(len(idx), generator=self.gen_times) if self.stage.draws_times else None
        losses = self.stage.step(idx, times)
        self.pending.append((self.iter, epoch, lr, losses))
        self.iter += 1
        return losses

    def flush(self):
        """Read the pending losses (one device->host copy), append one JSON line per step to loss.jsonl, print a
        summary, and raise FloatingPointError on a non-finite value."""
        if not self.pending:
            return []
        keys = list(self.pending[0][3])
        flat = torch.stack([torch.as_tensor(l[k]).detach().double().reshape(()) for _, _, _, l in self.pending
                            for k in keys])
        vals = flat.cpu().reshape(len(self.pending), len(keys)).tolist()      # the one host read of the window
        seconds = (time.perf_counter() - self._window_t0) / len(self.pending)
        rows = [dict(iter=it, epoch=ep, lr=lr, seconds=seconds, **dict(zip(keys, v)))
                for (it, ep, lr, _), v in zip(self.pending, vals)]
        self.pending, self._window_t0 = [], None
        bad = [r for r in rows if not all(math.isfinite(r[k]) for k in keys)]
        if self.rank == 0:
            with open(os.path.join(self.dir, 'loss.jsonl'), 'a') as fh:
                for r in rows:
                    fh.write(json.dumps(r) + '\n')
            last = rows[-1]
            print('iter %d epoch %d lr %.3e  %s  (%.3f s/step over %d steps)'
                  % (last['iter'], last['epoch'], last['lr'],
                     '  '.join('%s %.5f' % (k, sum(r[k] for r in rows) / len(rows)) for k in keys), seconds, len(rows)),
                  flush=True)
        if bad:
            raise FloatingPointError('non-finite loss at iteration %d: %s' % (bad[0]['iter'], bad[0]))
        return rows

    def run(self):
        a = self.args
        while self.iter < self.total_iters:
            self.step()
            if self.iter % a.print_freq == 0:
                self.flush()
            if self.iter % a.save_steps_freq == 0:
                self.save('steps-latest')
                self.save('steps-%d' % self.iter)
            elif self.iter % a.save_latest_freq == 0:
                self.save('steps-latest')
        self.flush()
        if self.iter % a.save_latest_freq != 0 and self.iter % a.save_steps_freq != 0:
            self.save('steps-latest')                           # the end of the run is always resumable
        return self.iter


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.train', description=__doc__.split('\n\n')[0])
    ap.add_argument('--model', required=True, choices=MODELS)
    ap.add_argument('--config', default='snet_uncond', choices=sorted(configs.CONFIGS))
    ap.add_argument('--dataset-dir', required=True, help='holds <name>/pointcloud.npz (and sdf.npz for --model vae)')
    ap.add_argument('--names', required=True, metavar='FILE', help='one `<name> [<label>]` per line')
    ap.add_argument('--logs-dir', default='logs')
    ap.add_argument('--name', default='experiment')
    ap.add_argument('--epochs', type=int, default=4000)
    ap.add_argument('--batch', type=int, default=4, help='shapes per step and rank')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--update-learning-rate', action='store_true', help='half-cosine per epoch (diffusion stages)')
    ap.add_argument('--min-lr', type=float, default=1e-6)
    ap.add_argument('--warmup-epochs', type=float, default=0)
    ap.add_argument('--ema-rate', type=float, default=0.999)
    ap.add_argument('--vae', default=None, help='GraphVAE checkpoint (stages hr of a 2-stage config, feature)')
    ap.add_argument('--pretrain-ckpt', default=None, help='df_*.pth holding the earlier, frozen stages')
    ap.add_argument('--ckpt', default=None, help='checkpoint to continue from (default: <logs>/<name>/ckpt/*_steps-latest.pth)')
    ap.add_argument('--print-freq', type=int, default=25)
    ap.add_argument('--save-latest-freq', type=int, default=500)
    ap.add_argument('--save-steps-freq', type=int, default=1000)
    ap.add_argument('--ckpt-num', type=int, default=5)
    ap.add_argument('--point-scale', type=float, default=0.5)
    ap.add_argument('--point-sample-num', type=int, default=50000, help='SDF samples per shape (--model vae)')
    ap.add_argument('--no-fused', dest='fused', action='store_false',
                    help='per-tensor optimiser launches and a host read of the loss every step')
    return ap


def main(argv=None, config=None, vae_config=None):
    """The command line.  config / vae_config: dicts for in-process callers (--config stays restricted to
    configs.CONFIGS)."""
    from . import _lib, dist
    args = parser().parse_args(argv)
    _lib.require_device()
    rank, _local_rank, world = dist.init()
    tr = Trainer(args, config=config, vae_config=vae_config, rank=rank, world=world)
    if rank == 0:
        print('train: %s, %d names, %d steps per epoch, starting at step %d of %d'
              % (args.model, len(tr.names), tr.epoch_length, tr.iter, tr.total_iters))
    done = tr.run()
    dist.barrier()
    return done


if __name__ == '__main__':
    main()
